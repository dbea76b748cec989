"""Gradients of a resident batch (gar_hip_adjoint_async, csrc/gar_adjoint.hpp) at the headline size:
(36, 12), N = 256, batch 4 096, device-generated problems in mode "F" (A uniform in [-1, 1], a singular Q), beside the
full solve of the same solver in the same process.  One JSON line with, HIP events on the solver's stream, best of REPS
after warm-up (ms):
  backward_forward_ms   backward + forward: the unit
  solve_ms              adjoint_async with neither output, W cached: scatter + sweep + initial stage + roll-out
  whole_ms              adjoint_async with the gradient records and no adjoint vectors: the same launches + the gradient
                        kernel
  gradients_ms          BY DIFFERENCE, whole_ms - solve_ms: the one launch the two windows differ by, gar_adjoint_gradients
                        (the kernel timed on its own: scripts/ubench/grad_store_forms.cpp, same geometry)
  gather_ms             BY DIFFERENCE: what asking for the adjoint vectors adds (gar_solution_gather)
  prepare_ms            what the FIRST adjoint after a backward adds (gar_affine_prepare forms W)
and the gradient kernel's write walk -- batch x (N + 1) records of the caller's knot size (+ G0 | g0) -- as a fraction of
what 8 TB/s and the 6.29 TB/s of a plain copy would move in gradients_ms.
The timed window is the library's default schedule for the batch; a device is required.
  python scripts/bench_adjoint.py [--reps 10] [--batch 4096] [--horizon 256]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aligator_amd import synth_device                             # noqa: E402
from aligator_amd.gar import BatchedRiccatiSolver                  # noqa: E402

MUEQ = 1e-10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=256)
    a = ap.parse_args()
    import torch
    nx, nu, N, batch = 36, 12, a.horizon, a.batch
    dims = [(nx, nu, 0, nx, 0)] * N + [(nx, 0, 0, nx, 0)]
    s = BatchedRiccatiSolver(dims, nx, batch=batch)
    synth_device.fill_problems(s, seed=5, mode="F", keep=())
    stream = torch.cuda.Stream()
    s.set_stream(stream.cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(7)
    cot = torch.randn((batch, s.affine_doubles), dtype=torch.float64, device="cuda", generator=gen)
    adj = torch.empty_like(cot)
    grad = torch.empty((batch, s.problem_doubles), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.sync()
        e0.record(stream)
        fn()
        s.device_pointers()           # (orders the solver's stream behind the half streams of a pipelined sweep; no host wait)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def solve():
        s.backward_async(MUEQ)
        s.forward_async()
    solve_only = lambda: s.adjoint_async(cot.data_ptr(), 0, 0)
    with_vectors = lambda: s.adjoint_async(cot.data_ptr(), adj.data_ptr(), 0)
    whole = lambda: s.adjoint_async(cot.data_ptr(), 0, grad.data_ptr())
    for _ in range(2):                                                # warm-up: every kernel of the timed windows
        solve(); whole(); solve_only(); with_vectors()
    s.sync()
    assert s.num_failed() == 0
    t = dict(backward_forward=[], first=[], solve=[], vectors=[], whole=[])
    for _ in range(a.reps):
        t["backward_forward"].append(timed(solve))
        t["first"].append(timed(solve_only))                          # (the first adjoint after a backward forms W)
        t["solve"].append(timed(solve_only))
        t["vectors"].append(timed(with_vectors))
        t["whole"].append(timed(whole))
    s.sync()
    finite = bool(torch.isfinite(grad).all().item() and torch.isfinite(adj).all().item())
    best = {k: min(v) for k, v in t.items()}
    grads = best["whole"] - best["solve"]
    out_bytes = 8 * batch * s.problem_doubles
    line = dict(shape=[nx, nu], horizon=N, batch=batch, kernel=s.kernel_name, pipeline=s.pipeline, reps=a.reps, mode="F",
                backward_forward_ms=best["backward_forward"], solve_ms=best["solve"], gradients_ms=grads,
                whole_ms=best["whole"], gather_ms=best["vectors"] - best["solve"], prepare_ms=best["first"] - best["solve"],
                solve_over_backward_forward=best["solve"] / best["backward_forward"],
                whole_over_backward_forward=best["whole"] / best["backward_forward"],
                gradient_bytes=out_bytes, gradient_bytes_per_stage=out_bytes / (batch * (N + 1)),
                gradients_frac_of_8TBs=out_bytes / (max(grads, 1e-9) * 8e9),
                gradients_frac_of_copy_6p29TBs=out_bytes / (max(grads, 1e-9) * 6.29e9),
                finite=finite, all_ms={k: [round(x, 4) for x in v] for k, v in t.items()})
    print(json.dumps(line), flush=True)
    s.close()


if __name__ == "__main__":
    main()
