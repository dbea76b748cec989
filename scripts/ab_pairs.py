"""Paired A/B of two library builds: alternating launches in one process, per-pair differences of the backward kernel.
usage: ab_pairs.py first=libX.so second=libY.so   (paths relative to aligator_amd/; launch order as given)"""
import ctypes as C, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aligator_amd import synth
from aligator_amd.gar import BatchedRiccatiSolver
libs = {a.split("=")[0]: os.path.join(ROOT, "aligator_amd", a.split("=")[1]) for a in sys.argv[1:]}
PAIRS = int(os.environ.get("AB_PAIRS", "8"))
nx, nu, N, mu = 36, 12, 256, 1e-14
for batch in (4096, 1024):
    for pipe in (0, -1):
        probs = [synth.generate_lq_problem(100 + i, np.zeros(nx), N, nx, nu, mode="W") for i in range(2)]
        solvers = {}
        for name, path in libs.items():
            s = BatchedRiccatiSolver([k.dims for k in probs[0].stages], nx, batch=batch, device=0, lib_path=path)
            packed = np.concatenate([s.pack(p) for p in probs])
            for b0 in range(0, batch, 2):
                s.upload_packed(packed, b0, 2)
            s.set_pipeline(pipe)
            s._check(s._L.gar_hip_set_timing(s.handle, 1))
            for _ in range(2):
                s.backward_async(mu); s.forward_async()
            s.sync()
            solvers[name] = s
        times = {k: [] for k in solvers}
        import time
        wall = {k: [] for k in solvers}
        for rep in range(PAIRS):
            for name, s in solvers.items():
                t0 = time.perf_counter()
                s.backward_async(mu); s.forward_async(); s.sync()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                o = (C.c_double * 3)(); s._check(s._L.gar_hip_last_kernel_ms(s.handle, o))
                times[name].append((o[0], o[2]))
        names = list(solvers)
        a, b = np.array(times[names[0]]), np.array(times[names[1]])
        for nm, t in ((names[0], a), (names[1], b)):
            print(f"batch {batch} pipeline {solvers[nm].pipeline} {solvers[nm].kernel_name} {nm:7s} backward ms "
                  + " ".join(f"{v:.3f}" for v in t[:, 0]) + f" | mean {t[:, 0].mean():.3f}  forward mean {t[:, 1].mean():.3f}"
                  f"  wall step mean {np.mean(wall[nm]):.3f}  failed {solvers[nm].num_failed()}", flush=True)
        d = a[:, 0] - b[:, 0]
        print(f"   per-pair backward difference {names[0]} - {names[1]}: mean {d.mean():+.4f} ms  std {d.std(ddof=1):.4f}  "
              f"mean/std {abs(d.mean()) / d.std(ddof=1):.1f}  ({100 * d.mean() / a[:, 0].mean():+.2f} % of {names[0]})", flush=True)
        w = np.array(wall[names[0]]) - np.array(wall[names[1]])
        print(f"   per-pair wall step difference: mean {w.mean():+.4f} ms  std {w.std(ddof=1):.4f}", flush=True)
        x = [solvers[k].solution(1) for k in solvers]
        same = all(np.array_equal(p, q) for A, B in zip(*x) for p, q in zip(A, B))
        print(f"   solutions of problem 1 bitwise identical: {same}", flush=True)
        for s in solvers.values():
            s.close()
