"""A resident batch solved for many affine terms at once (gar_hip_affine_solve_multi_async, csrc/gar_affine_multi.hpp,
DESIGN.md 5.3f) at the headline size: (36, 12), N = 256, device-generated problems in mode "F" (A uniform in [-1, 1], a
singular Q), against the calls it replaces -- nrhs successive adjoint_async(cot, adj, 0), one column each -- on the same
solver in the same process, W cached in both.  The batch is the largest of 4 096 and 1 024 whose buffers (the work buffers
of the header's formula, rhs and out for 64 columns) fit beside the solver; --batch fixes it.
One JSON line, HIP events on the solver's stream, best of REPS after warm-up (ms); within a repetition the launches
alternate: single x 16, multi 16, single x 16 again, multi 64, single x 64.
  single16_ms, single16_again_ms   16 successive single-column calls, the two series; single_spread_ms their difference
  multi16_ms, multi64_ms           ONE call with nrhs = 16 / 64
  single64_ms                      64 successive single-column calls
  faster_at_16                     multi16_ms < min(single16) - single_spread_ms: the acceptance of DESIGN.md 5.3f
  ratio16, ratio64                 single / multi
  bytes_per_column                 what the two paths walk per column and stage, counted from the layouts (kernel by kernel)
The per-kernel times come from a second run under a kernel trace (scripts/README.md has the command).
  timeout -k 10 600 python scripts/bench_affine_multi.py --batch 4096 && timeout -k 10 300 python scripts/bench_affine_multi.py --batch 1024
  python scripts/bench_affine_multi.py [--reps 10] [--batch 0 (choose)] [--horizon 256]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aligator_amd import synth_device                             # noqa: E402
from aligator_amd.gar import BatchedRiccatiSolver                  # noqa: E402

MUEQ = 1e-10
COLS = 16


def walk_bytes(nx, nu):
    """bytes per stage the kernels of the two paths move at (nx, nu, nx2 = nx), packed Vxx': per 16 columns for the panel
    path, per column for the single-column path (25 KB sweep, 19.6 KB roll-out)"""
    nr, vv = nu + nx, nx * (nx + 1) // 2
    mats_sweep, mats_roll, vec = vv + nr * nx + nu * nu + nx * nu, nr * nx + vv, 2 * nx + nu
    panel = dict(scatter=8 * 2 * COLS * vec, sweep=8 * (mats_sweep + 2 * COLS * vec),
                 rollout=8 * (mats_roll + COLS * (nr + nx) + COLS * vec))
    single = dict(scatter=8 * 2 * vec, sweep=8 * (mats_sweep + 2 * vec), rollout=8 * (mats_roll + (nr + nx) + 2 * vec),
                  gather=8 * 2 * vec)
    return panel, single


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--horizon", type=int, default=256)
    a = ap.parse_args()
    import torch
    nx, nu, N = 36, 12, a.horizon
    dims = [(nx, nu, 0, nx, 0)] * N + [(nx, 0, 0, nx, 0)]
    n_aff = (N + 1) * 2 * nx + N * nu + nx

    def extra_bytes(batch):          # the header's formula (P = 1 at these batches) + rhs and out of 64 and of 16 columns, cot and adj
        work = batch * 8 * ((N + 1) * 2 * COLS * (2 * nx + nu) + COLS * 3 * 2 * nx)
        return work + 2 * (64 + 16 + 1) * batch * n_aff * 8

    s, batch = None, 0
    for cand in ([a.batch] if a.batch else [4096, 1024]):
        s = BatchedRiccatiSolver(dims, nx, batch=cand)
        free, _ = torch.cuda.mem_get_info()
        # (the solver's own lazily allocated side buffers -- W, the refinement's and the adjoint's -- are about 4 GB at 4 096)
        if a.batch or free > extra_bytes(cand) + cand * (8 << 20) // 4:
            batch = cand
            break
        s.close()
        s = None
    assert s is not None, "neither batch fits"
    synth_device.fill_problems(s, seed=5, mode="F", keep=())
    stream = torch.cuda.Stream()
    s.set_stream(stream.cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(7)
    rhs = torch.randn((batch, 64, s.affine_doubles), dtype=torch.float64, device="cuda", generator=gen)
    out = torch.empty_like(rhs)
    rhs16 = rhs[:, :16].contiguous()
    out16 = torch.empty_like(rhs16)
    cot = rhs[:, 0].contiguous()
    adj = torch.empty_like(cot)
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.sync()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def singles(n):
        def run():
            for _ in range(n):
                s.adjoint_async(cot.data_ptr(), adj.data_ptr(), 0)
        return run
    multi16 = lambda: s.affine_solve_multi_async(rhs16.data_ptr(), 16, out16.data_ptr())
    multi64 = lambda: s.affine_solve_multi_async(rhs.data_ptr(), 64, out.data_ptr())
    s.backward_async(MUEQ)
    s.forward_async()
    for _ in range(2):                                                # warm-up: every kernel of the timed windows, W formed
        singles(2)(); multi16(); multi64()
    s.sync()
    assert s.num_failed() == 0
    t = dict(single16=[], multi16=[], single16_again=[], multi64=[], single64=[])
    for _ in range(a.reps):
        t["single16"].append(timed(singles(16)))
        t["multi16"].append(timed(multi16))
        t["single16_again"].append(timed(singles(16)))
        t["multi64"].append(timed(multi64))
        t["single64"].append(timed(singles(64)))
    s.sync()
    # column 0 of the multi-column result against the single-column path's (sums ordered differently: not bitwise)
    agree = float((out16[:, 0] - adj).abs().max().item() / max(1.0, adj.abs().max().item()))
    finite = bool(torch.isfinite(out).all().item() and torch.isfinite(out16).all().item())
    best = {k: min(v) for k, v in t.items()}
    spread = abs(best["single16"] - best["single16_again"])
    single16 = min(best["single16"], best["single16_again"])
    panel, single = walk_bytes(nx, nu)
    stages = batch * (N + 1)
    line = dict(shape=[nx, nu], horizon=N, batch=batch, kernel=s.kernel_name, pipeline=s.pipeline, reps=a.reps, mode="F",
                single16_ms=best["single16"], single16_again_ms=best["single16_again"], single_spread_ms=spread,
                multi16_ms=best["multi16"], multi64_ms=best["multi64"], single64_ms=best["single64"],
                faster_at_16=bool(best["multi16"] < single16 - spread),
                ratio16=single16 / best["multi16"], ratio64=best["single64"] / best["multi64"],
                bytes_per_stage_per_16_columns=panel, bytes_per_stage_per_column_single=single,
                bytes_per_column=dict(panel=sum(panel.values()) / COLS, single=sum(single.values())),
                walk_ms_at_8TBs=dict(multi16={k: v * stages / 8e9 for k, v in panel.items()},
                                     single16={k: 16 * v * stages / 8e9 for k, v in single.items()}),
                multi16_frac_of_walk_at_8TBs=sum(panel.values()) * stages / 8e9 / best["multi16"],
                single16_frac_of_walk_at_8TBs=16 * sum(single.values()) * stages / 8e9 / single16,
                column0_against_single=agree, finite=finite, all_ms={k: [round(x, 4) for x in v] for k, v in t.items()})
    print(json.dumps(line), flush=True)
    s.close()


if __name__ == "__main__":
    main()
