"""The serial fold (GAR_HIP_SERIAL_FOLD=1) against the any-dimension kernels, on the pattern it was built
for: a goal constraint on the terminal knot only.  Two configurations, batch 1 024:
  (36, 12), N = 256, nc = 6 on the terminal knot;   (56, 24), N = 275, nc = 8 on the terminal knot.
Per configuration: sweeps/s with the switch on, with it off (the any-dimension kernels: what a solver without the switch
runs for these dimensions), and the fold pass's own time = the backward kernels' time of the fold solver minus that of an
unconstrained solver of the same shape on the same knots (gar_hip_set_timing brackets the fold + the family's sweep).
Warm-up, then STEPS timed steps each; medians.  The problems are generated on the host (aligator_amd/synth_device.py
emits constraints on every knot or on none), DISTINCT of them, repeated over the batch.
  python scripts/bench_serial_fold.py [--batch 1024] [--steps 20] [--distinct 64]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aligator_amd import synth                                    # noqa: E402
from aligator_amd.gar import BatchedRiccatiSolver, lqrComputeKktError   # noqa: E402
from aligator_amd.lqr import LqrProblem                           # noqa: E402

MUEQ = 1e-6


def problems(nx, nu, N, nc_term, count):
    out = []
    for i in range(count):
        rng = np.random.default_rng([7, nx, nu, i])
        knots = [synth.generate_knot(rng, nx, nu, 0, singular=False, mode="W") for _ in range(N)]
        term = synth.generate_knot(rng, nx, 0, nc_term, singular=False, mode="W")
        term.C[...] = rng.uniform(-1, 1, term.C.shape)
        p = LqrProblem(knots + [term], nx)
        p.G0[...] = -np.eye(nx)
        p.g0[...] = rng.standard_normal(nx)
        out.append(p)
    return out


def solver(probs, batch, env):
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        s = BatchedRiccatiSolver([k.dims for k in probs[0].stages], probs[0].nc0, batch=batch)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    packed = np.concatenate([s.pack(p) for p in probs])
    for b0 in range(0, batch, len(probs)):
        s.upload_packed(packed, b0, min(len(probs), batch - b0))
    return s


def timed(s, steps, warmup=3):
    """-> (median seconds per backward + forward step, median ms of the backward kernels)"""
    for _ in range(warmup):
        s.backward_async(MUEQ); s.forward_async()
    s.sync()
    assert s.num_failed() == 0
    dts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        s.backward_async(MUEQ); s.forward_async(); s.sync()
        dts.append(time.perf_counter() - t0)
    s._check(s._L.gar_hip_set_timing(s.handle, 1))
    kms, o = [], (C.c_double * 3)()
    for _ in range(steps):
        s.backward_async(MUEQ); s.forward_async(); s.sync()
        if s._L.gar_hip_last_kernel_ms(s.handle, o) == 0:
            kms.append(o[0])
    s._check(s._L.gar_hip_set_timing(s.handle, 0))
    return statistics.median(dts), (statistics.median(kms) if kms else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=64)
    a = ap.parse_args()
    for (nx, nu, N, nc) in ((36, 12, 256, 6), (56, 24, 275, 8)):
        probs = problems(nx, nu, N, nc, min(a.distinct, a.batch))
        line = dict(shape=[nx, nu], horizon=N, nc_terminal=nc, batch=a.batch, mueq=MUEQ, steps=a.steps)
        on = solver(probs, a.batch, {"GAR_HIP_SERIAL_FOLD": "1"})
        dt_on, k_on = timed(on, a.steps)
        kkt = max(lqrComputeKktError(probs[-1], *on.solution(len(probs) - 1), mueq=MUEQ))
        line.update(kernel_on=on.kernel_name, sweeps_per_s_on=a.batch / dt_on, ms_per_step_on=dt_on * 1e3, kkt_on=kkt,
                    backward_kernels_ms_on=k_on)
        del on
        try:
            off = solver(probs, a.batch, {"GAR_HIP_SERIAL_FOLD": None})
            dt_off, _ = timed(off, a.steps)
            line.update(kernel_off=off.kernel_name, sweeps_per_s_off=a.batch / dt_off, ms_per_step_off=dt_off * 1e3,
                        speedup=dt_off / dt_on)
            del off
        except RuntimeError as e:       # (56, 24) with constraints: the any-dimension kernels do not fit a CU's LDS
            line.update(kernel_off=None, off_error=str(e))
        plain = [LqrProblem(p.stages[:-1] + [synth.generate_knot(np.random.default_rng(1), nx, 0, 0, mode="W")], nx)
                 for p in probs]
        for p, q in zip(plain, probs):
            p.G0[...], p.g0[...] = q.G0, q.g0
        unc = solver(plain, a.batch, {"GAR_HIP_SERIAL_FOLD": None})
        dt_unc, k_unc = timed(unc, a.steps)
        line.update(kernel_unconstrained=unc.kernel_name, sweeps_per_s_unconstrained=a.batch / dt_unc,
                    backward_kernels_ms_unconstrained=k_unc)
        if k_on is not None and k_unc is not None:
            line.update(fold_pass_ms=k_on - k_unc, fold_pass_over_unconstrained_step=(k_on - k_unc) / (dt_unc * 1e3))
        del unc
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
