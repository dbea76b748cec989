"""The serial fold (GAR_HIP_SERIAL_FOLD=1; csrc/gar_fold.hpp): cases and checks shared by the emulator
tests (tests/test_serial_fold.py) and the GPU tests (tests/test_serial_fold_gpu.py).  A serial problem whose constrained
knots have D = 0 runs on the unconstrained serial family of its (nx, nu); everything is held against the oracle's serial
ProximalRiccatiSolver to the tolerance the leg fold is held to (parity_cases.check_constrained_legs_fold: 1e-8 relative,
the multipliers against what the problem's conditioning allows)."""
import contextlib
import inspect
import os

import numpy as np

from aligator_amd import _lib, synth
from aligator_amd.gar import BatchedRiccatiSolver, ParallelRiccatiSolver, lqrInitializeSolution, set_option
from aligator_amd.lqr import LqrProblem
import parity_cases as pc

TOL = inspect.signature(pc.check_constrained_legs_fold).parameters["tol"].default   # the fold's tolerance: 1e-8
MUEQS = (1e-6, 1e-2)

# (nx, nu), N, batch, {knot: nc}
CASES = {
    "A": (8, 4, 5, 3, {5: 3}),                           # terminal knot only: terminalSolve's fold, full-block terminal record
    "B": (8, 4, 5, 3, {1: 2, 3: 2, 5: 3}),               # mixed nc: two layouts, v offsets
    "C": (12, 4, 4, 2, {t: 5 for t in range(5)}),        # uniform nc that is no kConstrained row
    "D": (36, 12, 3, 2, {1: 32, 3: 6}),                  # headline family: packed Q / R out of the fold, packed Vxx into the expand
    "E": (56, 24, 3, 1, {3: 8}),                         # pair<>: 128-thread blocks
}
# the serial backward families of each shape (GAR_HIP_BACKWARD) and the name each binds
FAMILIES = {
    (8, 4): {"wave": "wave<8,4>", "wg4": "mfma<8,4>"},
    (12, 4): {"wave": "wave<12,4>", "wg4": "mfma<12,4>"},
    (36, 12): {"wave": "wave<36,12>", "wg4": "mfma<36,12>"},
    (56, 24): {"wave": "pair<56,24>"},                   # (the wide shape has the two-wave family alone)
}


def case_families(case):
    nx, nu = CASES[case][:2]
    return sorted(FAMILIES[(nx, nu)])


def make_problem(case, seed, pattern=None):
    nx, nu, N, _, nc = CASES[case]
    nc = nc if pattern is None else pattern
    rng = np.random.default_rng([seed, nx, nu, N])
    knots = [synth.generate_knot(rng, nx, nu if t < N else 0, nc.get(t, 0), singular=False, mode="W") for t in range(N + 1)]
    for k in knots:
        k.C[...] = rng.uniform(-1, 1, k.C.shape)        # a dense C; D stays zero
    prob = LqrProblem(knots, nx)
    prob.G0[...] = -np.eye(nx)
    prob.g0[...] = rng.standard_normal(nx)
    return prob


def make_batch(case, pattern=None):
    return [make_problem(case, 100 + b, pattern) for b in range(CASES[case][3])]


@contextlib.contextmanager
def options(lib_path=None, **kv):
    """Environment switches (GAR_HIP_<NAME>) for the solvers created inside; restored afterwards."""
    old = {k: os.environ.get("GAR_HIP_" + k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop("GAR_HIP_" + k, None)
            else:
                os.environ["GAR_HIP_" + k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop("GAR_HIP_" + k, None)
            else:
                os.environ["GAR_HIP_" + k] = v


def fold_on(family="wave"):
    return options(SERIAL_FOLD="1", BACKWARD=family)


def batched(probs, lib_path):
    p0 = probs[0]
    s = BatchedRiccatiSolver([k.dims for k in p0.stages], p0.nc0, batch=len(probs), lib_path=lib_path)
    s.upload(probs)
    return s


def fold_name(case, family):
    nx, nu = CASES[case][:2]
    return FAMILIES[(nx, nu)][family] + "+fold"


class _Factors:
    def __init__(self, s, b):
        self.s, self.b = s, b

    def __getitem__(self, t):
        return self.s.factor(t, self.b)


def assert_parity(s, probs, mueq, tol=TOL):
    """Solution (x, u, v, lambda) and every factor block of every problem of the batch against the oracle's serial solver;
    the getters: rows [K; Z; Lambda] of the gains, the full Vxx, kktMat from the caller's knots (compare_factors)."""
    for b, p in enumerate(probs):
        _, osol, ref = pc.oracle_serial(p, mueq)
        bound, _ = pc.conditioning_bound(p, mueq, ref)
        sc = pc.scale_of(ref)
        for A, B, bd in zip(s.solution(b), ref, bound):
            assert pc.maxdiff(A, B) <= max(tol, pc.CONDITIONING_MARGIN * bd) * sc, b
        s._mueq = mueq
        pc.compare_factors(_Factors(s, b), osol, p.horizon, tol, names=("ff", "fb"), vnames=("Vxx", "vx"))
        for t, k in enumerate(p.stages):
            f, o = s.factor(t, b), osol.datas(t)
            assert f.fb.shape == (k.nu + k.nc + k.nx2, k.nx) and f.vm.Vxx.shape == (k.nx, k.nx)
            assert np.array_equal(f.vm.Vxx, f.vm.Vxx.T) or np.abs(f.vm.Vxx - f.vm.Vxx.T).max() <= tol * np.abs(o.Vxx).max()
            if k.nc and not k.D.any():   # Z = C / mu in rows [nu, nu + nc)
                assert np.abs(f.fb[k.nu:k.nu + k.nc] - k.C / mueq).max() <= 1e-14 * np.abs(k.C / mueq).max()
        ff0, _, _, _ = s.initial(b)
        assert np.abs(ff0 - osol.kkt0_ff).max() <= tol * max(1.0, np.abs(osol.kkt0_ff).max())
        ffs, fbs = s.gains_all(b)      # the bulk read-back goes through the same expand step
        for t in range(p.horizon + 1):
            assert np.array_equal(fbs[t], s.factor(t, b).fb) and np.array_equal(ffs[t], s.factor(t, b).ff)


def check_case(case, family, mueq, lib_path=None):
    probs = make_batch(case)
    with fold_on(family):
        s = batched(probs, lib_path)
    assert s.kernel_name == fold_name(case, family), s.kernel_name
    assert s.record_format == 0                      # the caller-facing records: full blocks, row-major fb, full Vxx
    assert s.backward(mueq) and s.forward()
    assert s.num_failed() == 0
    assert_parity(s, probs, mueq)
    with options(SERIAL_FOLD=None, BACKWARD=family):
        if CASES[case][:2] == (56, 24):
            # the any-dimension kernels do not fit a CU's LDS at (56, 24) with constraints: without the switch there is no
            # solver for these dimensions at all (and with it, none for a problem with D != 0: reported as failed)
            import pytest
            with pytest.raises(RuntimeError, match="LDS"):
                batched(probs, lib_path)
        else:
            off = batched(probs, lib_path)
            assert off.kernel_name == "generic", off.kernel_name
    return s


def bitwise_equal(s1, b1, s2, b2, horizon):
    for A, B in zip(s1.solution(b1), s2.solution(b2)):
        for a, b in zip(A, B):
            assert np.array_equal(a, b)
    for t in range(horizon + 1):
        f, g = s1.factor(t, b1), s2.factor(t, b2)
        for a, b in ((f.ff, g.ff), (f.fb, g.fb), (f.vm.Vxx, g.vm.Vxx), (f.vm.vx, g.vm.vx)):
            assert np.array_equal(a, b), t
    assert np.array_equal(s1.initial(b1)[0], s2.initial(b2)[0])


def check_fallback_bitwise(lib_path=None, family="wave", mueq=1e-6):
    """Case F: pattern B, problem 1 of 3 has a random D on knot 3 -- it is the any-dimension kernels' bit for bit, the
    other two are what they are in a batch without it."""
    probs = make_batch("B")
    plain = [p.copy() for p in probs]
    rng = np.random.default_rng(5)
    probs[1].stages[3].D[...] = rng.uniform(-1, 1, probs[1].stages[3].D.shape)
    N = probs[0].horizon
    with fold_on(family):
        s = batched(probs, lib_path)
        ref = batched(plain, lib_path)
    with options(FORCE_GENERIC="1", SERIAL_FOLD=None):
        gen = batched([probs[1]], lib_path)
    assert s.kernel_name == fold_name("B", family) and gen.kernel_name == "generic"
    for q in (s, ref, gen):
        assert q.backward(mueq) and q.forward() and q.num_failed() == 0
    bitwise_equal(s, 1, gen, 0, N)
    bitwise_equal(s, 0, ref, 0, N)
    bitwise_equal(s, 2, ref, 2, N)
    assert_parity(s, probs, mueq)


def check_mueq_zero(lib_path=None, family="wave"):
    """Case G: pattern A at mueq = 0 -- the constrained terminal knot divides by it (riccati-kernel.hxx:146-149): refused
    as the failed stage it is, like on a leg-fold solver.  And with the constraint on knot 1 alone: the fold flags every
    problem, the any-dimension kernels meet the singular [Rhat 0; 0 0] and report it as the reference does.  Neither
    poisons the solver."""
    for pattern in (None, {1: 3}):
        probs = make_batch("A", pattern)[:2]
        assert not pc.reference_solvable(probs[0], 0.0)
        with fold_on(family):
            s = batched(probs, lib_path)
        assert s.kernel_name == fold_name("A", family)
        pc.assert_reported_failure(s.backward, 0.0)
        assert s.backward(1e-6) and s.forward() and s.num_failed() == 0
        assert_parity(s, probs, 1e-6)


def check_against_leg_fold(lib_path=None, family="wave", mueq=1e-6):
    """Case B on the serial fold and on the 2-leg fold (no download of the folded buffer exists: the solutions compared)."""
    prob = make_problem("B", 100)
    with fold_on(family):
        s = batched([prob], lib_path)
    assert s.backward(mueq) and s.forward()
    par = ParallelRiccatiSolver(prob.copy(), 2, lib_path=lib_path)
    assert par.kernel_name.startswith("wave_leg<8,4>+fold"), par.kernel_name
    sol = lqrInitializeSolution(prob)
    assert par.backward(mueq) and par.forward(*sol)
    _, _, ref = pc.oracle_serial(prob, mueq)
    bound, _ = pc.conditioning_bound(prob, mueq, ref)
    sc = pc.scale_of(ref)
    for A, B, bd in zip(s.solution(0), sol, bound):
        assert pc.maxdiff(A, B) <= max(TOL, pc.CONDITIONING_MARGIN * bd) * sc


def check_switch(lib_path=None):
    """set_option is accepted; "0" right before create: generic, bit for bit what a solver gets with the switch unset."""
    probs = make_batch("A")
    N = probs[0].horizon
    with options(SERIAL_FOLD=None, BACKWARD="wave"):
        unset = batched(probs, lib_path)
        try:
            set_option("SERIAL_FOLD", "1", lib_path)         # raises where the library does not know the switch
            on = batched(probs, lib_path)
            set_option("SERIAL_FOLD", "0", lib_path)
            off = batched(probs, lib_path)
        finally:
            set_option("SERIAL_FOLD", None, lib_path)
    assert on.kernel_name == fold_name("A", "wave") and off.kernel_name == "generic" and unset.kernel_name == "generic"
    for q in (unset, off):
        assert q.backward(1e-6) and q.forward()
    bitwise_equal(off, 0, unset, 0, N)
    bitwise_equal(off, 2, unset, 2, N)


def check_cycle_append(lib_path=None, family="wave", mueq=1e-6):
    """One cycle on case B (the dimensions change: both layouts are rebuilt) and on case C (uniform: both layouts turn as
    a ring and only the new knot is uploaded), then parity again."""
    for case in ("B", "C"):
        nx, nu, N, _, pattern = CASES[case]
        probs = make_batch(case)
        with fold_on(family):
            s = batched(probs, lib_path)
            assert s.backward(mueq) and s.forward()
            rng = np.random.default_rng(9)
            nc_new = pattern.get(0, 0)                       # the knot that leaves comes back in: the pattern turns
            s.cycle_append((nx, nu, nc_new, nx, 0))
            for b, p in enumerate(probs):
                new = synth.generate_knot(rng, nx, nu, nc_new, singular=False, mode="W")
                new.C[...] = rng.uniform(-1, 1, new.C.shape)
                p.stages[:N] = p.stages[1:N] + [new]
                if case == "C":
                    s.upload_knot(b, N - 1, new)
            if case == "B":
                s.upload(probs)
        assert s.kernel_name == fold_name(case, family), s.kernel_name
        assert s.backward(mueq) and s.forward() and s.num_failed() == 0
        assert_parity(s, probs, mueq)


def check_pipeline_refused(lib_path=None):
    import pytest
    with fold_on("wave"):
        s = batched(make_batch("A"), lib_path)
    with pytest.raises(RuntimeError, match="gar_hip error -3"):     # GAR_HIP_ERR_UNSUPPORTED
        s.set_pipeline(2)
    assert s.pipeline == 0
    s.set_pipeline(-1)                                                  # the library's own choice: never an error, off
    assert s.pipeline == 0


def check_no_allocation(lib_path=None, rounds=3):
    L = _lib.load(lib_path)
    probs = make_batch("B")
    with fold_on("wave"):
        s = batched(probs, lib_path)
    assert s.backward(1e-6) and s.forward()
    s.fetch_results(0)
    s.factor(1, 0).kktMat
    before = L.gar_hip_debug_alloc_count()
    assert before > 0
    for _ in range(rounds):
        for b, p in enumerate(probs):
            for t, k in enumerate(p.stages):
                s.upload_knot(b, t, k)
            s.set_init(b, p.G0, p.g0)
        assert s.backward(1e-6) and s.forward()
        s.fetch_results(0)
        s.solution(1)
    assert L.gar_hip_debug_alloc_count() == before, L.gar_hip_debug_alloc_count() - before


def check_update_lq(lib_path=None, device=False, mueq=1e-2):
    """Case A's dimensions assembled on the device (gar_hip_update_lq_subproblem_device writes the caller-facing knots, C
    and d included), then backward, forward, parity."""
    from test_update_lq import random_derivs
    from aligator_amd.lqr import LqrKnot
    from oracle.update_lq import update_lq_subproblem
    nx, nu, N, batch, pattern = CASES["A"]
    dims = [(nx, nu if t < N else 0, pattern.get(t, 0), nx, 0) for t in range(N + 1)]
    rng = np.random.default_rng(77)
    with fold_on("wave"):
        s = BatchedRiccatiSolver(dims, nx, batch=batch, lib_path=lib_path)
    assert s.kernel_name == fold_name("A", "wave")
    probs, bufs = [], []
    for b in range(batch):
        derivs, init = random_derivs(rng, dims, nx)
        bufs.append(s.pack_derivs(derivs, init))
        prob = LqrProblem([LqrKnot(*d[:4]) for d in dims], nx)
        update_lq_subproblem(prob, derivs, init, 1e-6, True)
        probs.append(prob)
    flat = np.concatenate(bufs)
    if device:
        import torch
        dev = torch.from_numpy(flat).cuda()
        torch.cuda.synchronize()
        ptr = dev.data_ptr()
    else:
        ptr = flat.ctypes.data
    s.update_lq_subproblem_device(ptr, 1e-6, True)
    s.sync()
    packed = s.download_packed()
    for b, prob in enumerate(probs):
        assert np.array_equal(packed[b * s.problem_doubles:(b + 1) * s.problem_doubles], s.pack(prob))
    assert s.backward(mueq) and s.forward() and s.num_failed() == 0
    assert_parity(s, probs, mueq)
