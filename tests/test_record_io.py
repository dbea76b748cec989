"""How a caller's blocks map onto the device's records (aligator_amd/csrc/gar_record_io.hpp), from three sides.

* tests/unit/record_io_unit.cpp: the header alone -- put_block, take_block, the knot and initial-constraint maps, the
  gain-row function -- against element-by-element definitions, compiled with the host's AddressSanitizer and
  UndefinedBehaviorSanitizer (`make -C tests/unit record_io`; the program links the runtimes itself).
* On the wave emulator: both upload routes of the C ABI -- A: gar_hip_upload_stage x (N + 1) + gar_hip_set_init,
  B: gar_hip_upload_packed -- over every record format (generic, packed Q / R, padded, padded + packed, leg mode, the
  constrained segment legs, several devices, a terminal knot given with nx2 = 0, user parameters): a second problem
  over a first one, then gar_hip_download_packed must give pack(second) bit for bit; on padded solvers the emulated
  device record itself is compared with the padded problem written out here (dummy Q = R = I, [G0 0; 0 -I], zeros).
* On the GPU (-m gpu): the same round trip where the emulator models nothing -- the pinned staging area, non-temporal
  stores and the fence ahead of the DMA engine's read, real asynchronous copies -- followed by a sweep whose KKT
  error is held to the tolerance the family's existing tests use."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from aligator_amd import synth
from aligator_amd.gar import BatchedRiccatiSolver, lqrComputeKktError, set_option
from aligator_amd.lqr import LqrKnot, LqrProblem
import parity_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "_build", "libgar_hip_emu.so")
UNIT = os.path.join(HERE, "unit")


def test_record_io_header_under_the_host_sanitizers():
    subprocess.run(["make", "-s", "-C", UNIT, "record_io"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(UNIT, "_build", "record_io_unit")], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "record io ok" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


# ---- problems ---------------------------------------------------------------------------------------------------------
def _problem(seed, nx, nu, N, nc=0, nth=0, coupled=False, term_nx2_0=False):
    rng = np.random.default_rng(seed)
    prob = synth.generate_lq_problem(rng, rng.standard_normal(nx), N, nx, nu, nth=nth, nc=nc, mode="W")
    if coupled:                                         # D != 0 on every knot: the constrained segment legs take it
        for k in prob.stages[:-1]:
            k.C[...] = rng.uniform(-1, 1, k.C.shape)
            k.D[...] = rng.uniform(-1, 1, k.D.shape)
    if term_nx2_0:                                      # SolverProxDDP's terminal knot: A is 0 x nx, f empty
        last = prob.stages[-1]
        term = LqrKnot(last.nx, 0, last.nc, 0)
        for name in ("Q", "q", "C", "d"):
            getattr(term, name)[...] = getattr(last, name)
        shrunk = LqrProblem(prob.stages[:-1] + [term], prob.nc0)
        shrunk.G0[...], shrunk.g0[...] = prob.G0, prob.g0
        prob = shrunk
    return prob


def _upload(s, prob, route, b=0):
    if route == "A":
        for t, k in enumerate(prob.stages):
            s.upload_knot(b, t, k)
        s.set_init(b, prob.G0, prob.g0)
    else:
        s.upload([prob], b0=b)


def _lower_packed(M):
    return np.concatenate([M[j:, j] for j in range(M.shape[0])]) if M.size else np.zeros(0)


def _padded_device_record(s, prob):
    """The device record of `prob` on the padded solver `s`, written out block by block; NaN where the record is
    not defined (the holes behind packed triangles, alignment gaps)."""
    want = np.full(s.device_problem_doubles, np.nan)
    nx, NX, nc0, NC0 = int(s.dims[0, 0]), int(s.device_dims[0, 0]), s.nc0, s.device_nc0
    assert NC0 - nc0 == NX - nx
    G = np.zeros((NC0, NX))
    G[:nc0, :nx] = prob.G0
    G[nc0:, nx:] = -np.eye(NX - nx)
    want[s.device_G0_off:s.device_G0_off + G.size] = G.ravel(order="F")
    want[s.device_g0_off:s.device_g0_off + NC0] = np.concatenate([prob.g0, np.zeros(NC0 - nc0)])
    for t, k in enumerate(prob.stages):
        NXt, NU, NC, NX2, _ = (int(v) for v in s.device_dims[t])
        assert NC == 0 and NX2 == NXt == NX and (NU > 0) == (k.nu > 0)

        def grown(blk, R, Cc, diag=0.0):
            blk = np.atleast_2d(blk.T).T if blk.ndim == 1 else blk
            out = np.zeros((R, Cc))
            out[:blk.shape[0], :blk.shape[1]] = blk
            for i in range(min(R - blk.shape[0], Cc - blk.shape[1])):
                out[blk.shape[0] + i, blk.shape[1] + i] = diag
            return out
        A = k.A if k.nx2 else np.zeros((nx, nx))            # (a terminal knot given with nx2 = 0)
        f = k.f if k.nx2 else np.zeros(nx)
        Q, R = grown(k.Q, NX, NX, 1.0), grown(k.R, NU, NU, 1.0)
        blocks = [Q, grown(k.S, NX, NU), R, grown(k.q, NX, 1), grown(k.r, NU, 1), grown(A, NX, NX), grown(k.B, NX, NU),
                  grown(f, NX, 1)]
        p = int(s.device_stage_offsets[t, 0])
        for i, blk in enumerate(blocks):
            flat = blk.ravel(order="F")
            if s.qr_packed and t < s.horizon and i in (0, 2):
                tri = _lower_packed(blk)
                want[p:p + tri.size] = tri
            else:
                want[p:p + flat.size] = flat
            p += flat.size
    return want


# name, (nx, nu, N), solver / problem keywords, what the row is there for
ROWS = [
    ("generic", (6, 3, 4), dict(env={"GAR_HIP_PAD": "0"}), dict(kernel="generic", padded=False, qr_packed=False)),
    ("packed_qr", (12, 4, 5), {}, dict(padded=False, qr_packed=True)),
    ("padded_4_2", (4, 2, 4), {}, dict(kernel="<8,4>", padded=True, qr_packed=True)),
    ("padded_7_3", (7, 3, 4), {}, dict(kernel="<8,4>", padded=True, qr_packed=True)),
    ("wide_56_22", (56, 22, 2), {}, dict(kernel="pair<56,24>", padded=True)),
    ("padded_legs", (12, 6, 7), dict(legs=3), dict(kernel="wave_leg<12,8>", padded=True)),
    ("wave_seg", (8, 4, 16), dict(legs=3, nc=4, coupled=True), dict(kernel="wave_seg<8,4,4>", padded=False, qr_packed=True)),
    ("wave_seg_2dev", (8, 4, 16), dict(legs=3, nc=4, coupled=True, devices=[0, 1]),
     dict(kernel="wave_seg<8,4,4>", padded=False, qr_packed=True)),
    ("padded_3dev", (6, 3, 13), dict(legs=3, devices=[0, 1, 2]), dict(padded=True)),
    ("terminal_nx2_0", (8, 4, 6), dict(term_nx2_0=True), dict(kernel="wave<8,4>", qr_packed=True)),
    ("terminal_nx2_0_padded", (6, 3, 5), dict(term_nx2_0=True), dict(kernel="<8,4>", padded=True)),
    ("user_parameters", (8, 4, 4), dict(nth=2), dict(padded=False)),
]


def _make(row, lib_path, seeds=(11, 12)):
    name, (nx, nu, N), kw, want = row
    pk = dict(nc=kw.get("nc", 0), nth=kw.get("nth", 0), coupled=kw.get("coupled", False),
              term_nx2_0=kw.get("term_nx2_0", False))
    probs = [_problem(seed + 100 * nx, nx, nu, N, **pk) for seed in seeds]
    s = BatchedRiccatiSolver([k.dims for k in probs[0].stages], probs[0].nc0, batch=1, num_legs=kw.get("legs", 1),
                             lib_path=lib_path, devices=kw.get("devices"))
    if "kernel" in want:
        assert want["kernel"] in s.kernel_name, s.kernel_name
    for flag in ("padded", "qr_packed"):
        if flag in want:
            assert getattr(s, flag) == want[flag], (flag, s.kernel_name)
    return s, probs


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu")], check=True)
    lib = C.CDLL(EMU)
    lib.emu_set_device_count(3)   # three virtual devices
    yield EMU
    lib.emu_set_device_count(1)


@pytest.mark.parametrize("route", ["A", "B"])
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_upload_routes_round_trip_bitwise_on_the_emulator(emu, monkeypatch, row, route):
    for k, v in row[2].get("env", {}).items():
        monkeypatch.setenv(k, v)
    s, (p1, p2) = _make(row, emu)
    rng = np.random.default_rng(3)
    p2.G0[...] = rng.uniform(-1, 1, p2.G0.shape)        # (nothing is solved here: any initial constraint will do)
    _upload(s, p1, route)
    assert np.array_equal(s.download_packed(), s.pack(p1))
    _upload(s, p2, route)
    back = s.download_packed()
    assert np.array_equal(back, s.pack(p2)), np.abs(back - s.pack(p2)).max()
    dev = s.device_pointers()[0]
    if s.padded and dev:                                # (a multi-device handle has no one device record)
        rec = np.frombuffer((C.c_double * s.device_problem_doubles).from_address(dev), dtype=np.float64)
        want = _padded_device_record(s, p2)
        known = ~np.isnan(want)
        assert 2 * known.sum() > want.size and np.array_equal(rec[known], want[known])
    s.close()


# ---- GPU ------------------------------------------------------------------------------------------------------------
GPU_ROWS = [
    ("wide_56_22_nt", (56, 22, 3), dict(option=("GAR_HIP_STAGE_NT", "1")), dict(kernel="pair<56,24>", padded=True)),
    ("wide_56_22_plain", (56, 22, 3), dict(option=("GAR_HIP_STAGE_NT", "0")), dict(kernel="pair<56,24>", padded=True)),
    # (one problem on a whole GPU binds the workgroup family, whose records are full: the one-wave family is asked for)
    ("packed_qr", (12, 4, 5), dict(option=("GAR_HIP_BACKWARD", "wave")), dict(kernel="wave<12,4>", padded=False, qr_packed=True)),
    ("padded_7_3", (7, 3, 4), dict(option=("GAR_HIP_BACKWARD", "wave")), dict(kernel="wave<8,4>", padded=True, qr_packed=True)),
    ("wave_seg_2dev", (8, 4, 16), dict(legs=3, nc=4, coupled=True, devices=[0, 0]),
     dict(kernel="wave_seg<8,4,4>", padded=False, qr_packed=True)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("row", GPU_ROWS, ids=[r[0] for r in GPU_ROWS])
def test_upload_routes_round_trip_bitwise_and_solve_on_the_gpu(row):
    """Tolerances: tests/test_abi_padding.py's check_raw_abi holds the unconstrained families to 1e-9 x the solution's
    scale (generator "W", mueq = 1e-10); the constrained segment legs are held to what their own test asks
    (parity_cases.check_constrained_legs_segments through check_parallel(conditioned=True), mueq = 1e-6):
    max(1e-8, CONDITIONING_MARGIN x the oracle's leg-parallel KKT error) x the scale."""
    kw = row[2]
    name, value = kw.get("option", (None, None))
    if name:
        set_option(name, value)
    try:
        s, (p1, p2) = _make(row, None)
    finally:
        if name:
            set_option(name, None)
    for route in ("A", "B"):
        _upload(s, p1, route)
        _upload(s, p2, route)
        assert np.array_equal(s.download_packed(), s.pack(p2)), route
    constrained = kw.get("nc", 0) > 0
    mueq = 1e-6 if constrained else 1e-10
    assert s.backward(mueq) and s.forward()
    sol = s.solution(0)
    _, _, ref = pc.oracle_serial(p2, mueq)
    sc = pc.scale_of(ref)
    ktol = 1e-9
    if constrained:
        from aligator_amd.lqr import lqrInitializeSolution
        from oracle import oracle as ora
        opar = ora.ParallelRiccatiSolver(pc.to_oracle(p2), kw["legs"])
        opar.backward(mueq)
        osol = lqrInitializeSolution(p2)
        opar.forward(*osol)
        ktol = max(1e-8, pc.CONDITIONING_MARGIN * max(lqrComputeKktError(p2, *osol, mueq=mueq)) / sc)
    kkt = max(lqrComputeKktError(p2, *sol, mueq=mueq))
    print(f"{row[0]}: kernel {s.kernel_name} kkt {kkt:.3e} bound {ktol * sc:.3e}")
    assert kkt <= ktol * sc
    s.close()
