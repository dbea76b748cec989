"""Paired A/B of library builds in the PIPELINED schedule, steady state: every build gets a solver of its own on the same
device-generated problems; launches alternate between the builds in one process.  One sample = K steps with no sync
between them (so both backward halves of the timed step run beside a roll-out), the library's events of the last step
(mean of the two gar_backward_wave_half launches, mean of the two gar_forward_lean launches) and the wall time per step.
Differences are taken per pair against the build named `parent` (the first one named, if there is none).
usage: ab_pipelined.py name=libX.so name=libY.so ...   (paths relative to aligator_amd/; launch order as given)
env: AB_PAIRS (10), AB_STEPS (3), AB_BATCH (4096)"""
import ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from aligator_amd import synth_device
from aligator_amd.gar import BatchedRiccatiSolver
libs = {a.split("=")[0]: os.path.join(ROOT, "aligator_amd", a.split("=")[1]) for a in sys.argv[1:]}
PAIRS = int(os.environ.get("AB_PAIRS", "10"))
STEPS = int(os.environ.get("AB_STEPS", "3"))
batch = int(os.environ.get("AB_BATCH", "4096"))
nx, nu, N, mu = 36, 12, 256, 1e-14
dims = [(nx, nu, 0, nx, 0)] * N + [(nx, 0, 0, nx, 0)]
solvers = {}
for name, path in libs.items():
    s = BatchedRiccatiSolver(dims, nx, batch=batch, device=0, lib_path=path)
    synth_device.fill_problems(s, seed=1, mode="W", keep=())
    s.set_pipeline(2)
    s._check(s._L.gar_hip_set_timing(s.handle, 1))
    for _ in range(2):
        s.backward_async(mu); s.forward_async()
    s.sync()
    solvers[name] = s
names = list(solvers)
bwd = {k: [] for k in names}; fwd = {k: [] for k in names}; wall = {k: [] for k in names}
for rep in range(PAIRS):
    for name in names:
        s = solvers[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            s.backward_async(mu); s.forward_async()
        s.sync()
        wall[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
        o = (C.c_double * 3)(); s._check(s._L.gar_hip_last_kernel_ms(s.handle, o))
        bwd[name].append(o[0]); fwd[name].append(o[2])
print(f"batch {batch} pipeline 2, {PAIRS} pairs of {STEPS} un-synced steps, launch order {' '.join(names)}", flush=True)
for nm in names:
    print(f"  {nm:8s} backward half ms " + " ".join(f"{v:.3f}" for v in bwd[nm]) + f" | mean {np.mean(bwd[nm]):.3f}"
          f"  roll-out half mean {np.mean(fwd[nm]):.3f}  wall ms/step mean {np.mean(wall[nm]):.3f}"
          f"  ({batch / np.mean(wall[nm]):.1f} k sweeps/s)  failed {solvers[nm].num_failed()}", flush=True)
ref = "parent" if "parent" in names else names[0]
x0 =solvers[ref].solution(1), solvers[ref].solution(batch - 1)
for nm in (n for n in names if n != ref):
    for what, tab in (("backward half", bwd), ("wall step", wall)):
        d = np.array(tab[nm]) - np.array(tab[ref])
        sd = d.std(ddof=1)
        print(f"  per-pair {what} difference {nm} - {ref}: mean {d.mean():+.4f} ms  std {sd:.4f}  |mean|/std {abs(d.mean()) / sd:.1f}"
              f"  ({100 * d.mean() / np.mean(tab[ref]):+.2f} %)", flush=True)
    x = solvers[nm].solution(1), solvers[nm].solution(batch - 1)
    same = all(np.array_equal(p, q) for A, B in zip(x0, x) for P, Q in zip(A, B) for p, q in zip(P, Q))
    print(f"  solutions of problems 1 and {batch - 1} bitwise those of {ref}: {same}", flush=True)
for s in solvers.values():
    s.close()
