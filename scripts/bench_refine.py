"""One refinement step from the stored factorisation (gar_hip_refine, csrc/gar_refine.hpp) at the headline
size: (36, 12), N = 256, batch 4 096, device-generated problems in mode "F" (A uniform in [-1, 1], a singular Q), beside
the full solve and the KKT evaluation of the same solver in the same process.  One JSON line with, HIP events on the
solver's stream, best of REPS after warm-up (ms):
  residual_ms           refine_async(0): ONE evaluation -- gar_kkt_stage_residuals with the residual vectors stored, and
                        the reduction with the gate words
  step_ms               refine_async(1) with W cached, minus residual_ms: one whole step (residual + sweep + initial stage
                        + roll-out); prepare_ms: what the FIRST step after a backward adds (gar_affine_prepare forms W)
  sweep_ms              NOT gar_refine_sweep but the RE-SOLVE's sweep, backward_affine_async with W cached: the same
                        code's other instance (gar_backward_affine) and the initial stage on the knots' own q, r, f,
                        standing in for the refinement's, which the ABI does not run alone (a kernel trace has both:
                        DESIGN.md 5.3d)
  rollout_ms            step_ms - residual_ms - sweep_ms: by difference against that stand-in
  kkt_error_ms          kkt_error_async, the evaluation without the vectors stored
  backward_forward_ms   backward + forward
and each kernel's byte walk counted from the layout (no cache effects) with the fraction of it 8 TB/s would move in the
measured time, and the batch maximum of the device triple before and after one and two steps.
The timed window is the library's default schedule for the batch; a device is required.
  python scripts/bench_refine.py [--reps 10] [--batch 4096] [--horizon 256]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aligator_amd import synth_device                             # noqa: E402
from aligator_amd.gar import BatchedRiccatiSolver                  # noqa: E402

MUEQ = 1e-10


def byte_walks(s):
    """(residual, sweep, roll-out) bytes per step for the whole batch, from the device layout"""
    N = s.horizon
    vp = bool(s.record_format & 2)
    res = swp = roll = 0
    for t in range(N + 1):
        nx, nu, nc, nx2, _ = (int(v) for v in s.device_dims[t])
        last = t == N
        n2 = 0 if last else nx2
        rows = nu if last else nu + nx2
        vxx = n2 * (n2 + 1) // 2 if vp else n2 * n2
        q = (nx * (nx + 1) // 2 + nu * (nu + 1) // 2) if (s.qr_packed and not last) else nx * nx + nu * nu
        # the residual: the knot and five solution vectors in; the four norms and gx | gu, dyn out
        res += q + nx * nu + nx + nu + (n2 * nx + n2 * nu + n2) + (2 * nx + nu + 2 * n2) + 4 + nx + nu + n2
        # the vector sweep: Vxx', fb, W, B, f~, q~ | r~ in; ff~, vx~ out
        swp += vxx + n2 * nu + n2 + rows * nx + nu * nu + nx + nu + rows + nx
        # the roll-out: fb, ff~, Vxx', vx~' in; u, x', lbda' read and written
        roll += rows * nx + rows + vxx + n2 + 2 * (nu + 2 * n2)
    return 8 * res * s.batch, 8 * swp * s.batch, 8 * roll * s.batch


def device_triples(s):
    import torch  # noqa: F401  (the HIP runtime torch already loaded)
    out = np.zeros((s.batch, 3))
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(s.device_kkt_errors()[0]), C.c_size_t(out.nbytes), 2) == 0
    return out


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
    for _ in range(2):                                                # warm-up: every kernel of the timed windows
        solve(); s.kkt_error_async(MUEQ); s.refine_async(1); s.backward_affine_async(); s.forward_async()
    s.sync()
    assert s.num_failed() == 0
    t = dict(backward_forward=[], kkt_error=[], residual=[], first_step=[], one_step=[], sweep=[])
    for _ in range(a.reps):
        t["backward_forward"].append(timed(solve))
        t["kkt_error"].append(timed(lambda: s.kkt_error_async(MUEQ)))
        t["residual"].append(timed(lambda: s.refine_async(0)))
        t["first_step"].append(timed(lambda: s.refine_async(1)))     # (the first step after a backward forms W)
        t["one_step"].append(timed(lambda: s.refine_async(1)))       # (two evaluations and one correction, W cached)
        t["sweep"].append(timed(s.backward_affine_async))
    solve()
    s.refine_async(0)
    s.sync()
    triples = [device_triples(s).max(axis=0)]
    for _ in range(2):
        s.refine_async(1)
        s.sync()
        triples.append(device_triples(s).max(axis=0))
    rb, sb, ob = byte_walks(s)
    best = {k: min(v) for k, v in t.items()}
    step = best["one_step"] - best["residual"]
    rollout = step - best["residual"] - best["sweep"]
    line = dict(shape=[nx, nu], horizon=N, batch=batch, kernel=s.kernel_name, pipeline=s.pipeline, reps=a.reps, mode="F",
                step_ms=step, residual_ms=best["residual"], sweep_ms=best["sweep"], rollout_ms=rollout,
                prepare_ms=best["first_step"] - best["one_step"],
                kkt_error_ms=best["kkt_error"], backward_forward_ms=best["backward_forward"],
                step_over_backward_forward=step / best["backward_forward"],
                residual_bytes=rb, sweep_bytes=sb, rollout_bytes=ob,
                rollout_bytes_per_stage=ob / (batch * (N + 1)),
                residual_frac_of_8TBs=rb / (best["residual"] * 8e9), sweep_frac_of_8TBs=sb / (best["sweep"] * 8e9),
                rollout_frac_of_8TBs=ob / (max(rollout, 1e-9) * 8e9),
                all_ms={k: [round(x, 4) for x in v] for k, v in t.items()},
                max_kkt_first_solve=[float(v) for v in triples[0]], max_kkt_one_step=[float(v) for v in triples[1]],
                max_kkt_two_steps=[float(v) for v in triples[2]])
    print(json.dumps(line), flush=True)
    s.close()


if __name__ == "__main__":
    main()
