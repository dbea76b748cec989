"""The device-side KKT residuals (gar_hip_kkt_error_async, csrc/gar_kkt.hpp) at the headline size and
for one problem: (36, 12), N = 256, batch 4 096 and batch 1.  Per configuration, one JSON line with
  kkt_ms              the KKT step (both kernels), HIP events on the solver's stream, best of REPS after warm-up;
  knot_bytes          the knot bytes the step reads (packed Q / R where the solver keeps them packed; the terminal
                      knot without A, B, f; G0, g0), computed from the layout; bytes_per_s = knot_bytes / kkt_ms;
  backward_ms         the backward sweep's kernel time on the same solver in the same run (gar_hip_last_kernel_ms:
                      per half-batch launch x 2 under the pipelined schedule) -- the yardstick: ratio = kkt_ms / backward_ms;
  copy_ceiling_ms     gar_hip_copy_ceiling_ms for the same byte count read (2 x knot_bytes moved: half read, half written).
The problems are generated on the device (aligator_amd/synth_device.py); a device is required.
  python scripts/bench_kkt_device.py [--reps 10] [--batch 4096 1] [--lib path/to/libgar_hip_variant.so]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aligator_amd import synth_device                             # noqa: E402
from aligator_amd.gar import BatchedRiccatiSolver                  # noqa: E402

MUEQ = 1e-10


def knot_bytes(s):
    """bytes of the records one KKT step fetches, per problem x batch (what gar_kkt_stage_residuals stages)"""
    total = s.device_nc0 * int(s.device_dims[0, 0]) + s.device_nc0
    N = s.horizon
    for t in range(N + 1):
        nx, nu, nc, nx2, _ = (int(v) for v in s.device_dims[t])
        packed = s.qr_packed and t < N
        total += (nx * (nx + 1) // 2 + nu * (nu + 1) // 2) if packed else (nx * nx + nu * nu)
        total += nx * nu + nx + nu + nc * nx + nc * nu + nc
        if t < N:
            total += nx2 * nx + nx2 * nu + nx2
    return 8 * total * s.batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, nargs="+", default=[4096, 1])
    ap.add_argument("--horizon", type=int, default=256)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    import torch
    nx, nu, N = 36, 12, a.horizon
    dims = [(nx, nu, 0, nx, 0)] * N + [(nx, 0, 0, nx, 0)]
    for batch in a.batch:
        s = BatchedRiccatiSolver(dims, nx, batch=batch, lib_path=a.lib)
        synth_device.fill_problems(s, seed=5, mode="W", keep=())
        stream = torch.cuda.Stream()
        s.set_stream(stream.cuda_stream)
        s._check(s._L.gar_hip_set_timing(s.handle, 1))
        out = (C.c_double * 3)()
        for _ in range(3):                                          # warm-up: every kernel of the timed window
            s.backward_async(MUEQ); s.forward_async(); s.kkt_error_async(MUEQ)
        s.sync()
        assert s.num_failed() == 0
        bwd, kkt = [], []
        for _ in range(a.reps):
            s.backward_async(MUEQ); s.forward_async(); s.sync()
            s._check(s._L.gar_hip_last_kernel_ms(s.handle, out))
            bwd.append(out[0] * (2 if s.pipeline == 2 else 1))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            s.kkt_error_async(MUEQ)
            e1.record(stream)
            e1.synchronize()
            kkt.append(e0.elapsed_time(e1))
        err = s.kkt_error(MUEQ)
        nbytes = knot_bytes(s)
        ceil = s._L.gar_hip_copy_ceiling_ms(0, 2 * nbytes, 5)
        line = dict(shape=[nx, nu], horizon=N, batch=batch, kernel=s.kernel_name, pipeline=s.pipeline, reps=a.reps,
                    lib=a.lib or "default", kkt_ms=min(kkt), kkt_ms_all=[round(v, 4) for v in kkt], knot_bytes=nbytes,
                    bytes_per_s=nbytes / (min(kkt) * 1e-3), backward_ms=min(bwd), ratio=min(kkt) / min(bwd),
                    copy_ceiling_ms=ceil, max_err=[float(v) for v in err.max(axis=0)])
        print(json.dumps(line), flush=True)
        s.close()


if __name__ == "__main__":
    main()
