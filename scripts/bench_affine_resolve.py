"""The re-solve for new affine terms (gar_hip_backward_affine, csrc/gar_affine.hpp) at the headline size:
(36, 12), N = 256, batch 4 096, beside the full sweep of the same solver in the same process.  One JSON line with, HIP
events on the solver's stream, best of REPS after warm-up (ms):
  prepare_ms            W = R-hat^-1 of every stage (gar_affine_prepare): the first re-solve after a backward minus a
                        later one, both timed whole
  affine_ms             backward_affine with W cached (the vector sweep + the stand-alone initial stage)
  affine_forward_ms     backward_affine + forward
  backward_ms           the full backward (sweep + initial stage), same stream, same events
  backward_forward_ms   backward + forward
  upload_ms             upload_affine_device (the scatter kernel)
and each step's byte walk, counted from the layout (what the kernels fetch and store, no cache effects), with the
fraction of it that 8 TB/s would move in the measured time:
  affine_bytes / prepare_bytes / backward_bytes, *_frac_of_8TBs = bytes / (ms * 8e9)
The timed window is the library's default schedule for the batch (pipelined at 4 096: the full sweep runs on the half
streams, the re-solve on the solver's stream behind them).  The problems are generated on the device
(aligator_amd/synth_device.py); a device is required.
  python scripts/bench_affine_resolve.py [--reps 10] [--batch 4096] [--horizon 256]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aligator_amd import synth_device                             # noqa: E402
from aligator_amd.gar import BatchedRiccatiSolver                  # noqa: E402

MUEQ = 1e-10


def byte_walks(s):
    """(affine, prepare, backward) bytes per call for the whole batch, from the device layout"""
    N = s.horizon
    vp = bool(s.record_format & 2)
    aff = prep = bwd = 0
    for t in range(N + 1):
        nx, nu, nc, nx2, _ = (int(v) for v in s.device_dims[t])
        nr = nu + nc + nx2
        vxx = nx2 * (nx2 + 1) // 2 if vp else nx2 * nx2
        own_vxx = nx * (nx + 1) // 2 if vp else nx * nx
        last = t == N
        # the vector sweep: Vxx', fb, W, B | f, q | r in; ff, vx out
        aff += (0 if last else vxx + nx2 * nu + nx2) + (nu if last else nr) * nx + nu * nu + nx + nu + (nu if last else nr) + nx
        # prepare: Vxx', B, R in; W out
        if nu:
            r = nu * (nu + 1) // 2 if (s.qr_packed and not last) else nu * nu
            prep += (0 if last else vxx + nx2 * nu) + r + nu * nu
        # the full stage: the knot in (packed Q, R where the family packs them), the factor record out, Vxx' | vx' in
        q = (nx * (nx + 1) // 2 + nu * (nu + 1) // 2) if (s.qr_packed and not last) else nx * nx + nu * nu
        knot = q + nx * nu + nx + nu + (0 if last else nx2 * nx + nx2 * nu + nx2)
        bwd += knot + nr + nr * nx + own_vxx + nx + (0 if last else vxx + nx2)
    return 8 * aff * s.batch, 8 * prep * s.batch, 8 * bwd * s.batch


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
    synth_device.fill_problems(s, seed=5, mode="W", keep=())
    stream = torch.cuda.Stream()
    s.set_stream(stream.cuda_stream)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    aff = torch.randn(batch, s.affine_doubles, generator=gen, device="cuda", dtype=torch.float64)
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

    def both(first, second):
        def fn():
            first()
            second()
        return fn
    for _ in range(2):                                                # warm-up: every kernel of the timed windows
        s.backward_async(MUEQ); s.forward_async(); s.upload_affine_device(aff.data_ptr())
        s.backward_affine_async(); s.forward_async(); s.backward_affine_async()
    s.sync()
    assert s.num_failed() == 0
    t = dict(first=[], affine=[], affine_forward=[], backward=[], backward_forward=[], upload=[])
    for _ in range(a.reps):
        t["backward"].append(timed(lambda: s.backward_async(MUEQ)))
        t["first"].append(timed(s.backward_affine_async))            # prepare + the vector sweep
        t["affine"].append(timed(s.backward_affine_async))
        t["affine_forward"].append(timed(both(s.backward_affine_async, s.forward_async)))
        t["backward_forward"].append(timed(both(lambda: s.backward_async(MUEQ), s.forward_async)))
        t["upload"].append(timed(lambda: s.upload_affine_device(aff.data_ptr())))
    s.backward_async(MUEQ); s.backward_affine_async(); s.forward_async(); s.sync()
    err = s.kkt_error(MUEQ)
    ab, pb, bb = byte_walks(s)
    best = {k: min(v) for k, v in t.items()}
    prepare = best["first"] - best["affine"]
    line = dict(shape=[nx, nu], horizon=N, batch=batch, kernel=s.kernel_name, pipeline=s.pipeline, reps=a.reps,
                prepare_ms=prepare, affine_ms=best["affine"], affine_forward_ms=best["affine_forward"],
                backward_ms=best["backward"], backward_forward_ms=best["backward_forward"], upload_ms=best["upload"],
                affine_over_backward=best["affine"] / best["backward"],
                affine_forward_over_backward_forward=best["affine_forward"] / best["backward_forward"],
                affine_bytes=ab, prepare_bytes=pb, backward_bytes=bb,
                affine_bytes_per_stage=ab / (batch * (N + 1)),
                affine_frac_of_8TBs=ab / (best["affine"] * 8e9), prepare_frac_of_8TBs=pb / (max(prepare, 1e-9) * 8e9),
                backward_frac_of_8TBs=bb / (best["backward"] * 8e9),
                all_ms={k: [round(x, 4) for x in v] for k, v in t.items()},
                max_kkt_after_resolve=[float(v) for v in err.max(axis=0)])
    print(json.dumps(line), flush=True)
    s.close()


if __name__ == "__main__":
    main()
