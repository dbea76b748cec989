"""Re-solve for new affine terms from the stored factorisation (gar_hip_backward_affine, csrc/gar_affine.hpp, DESIGN.md
5.3c): cases and checks shared by the emulator tests (tests/test_affine.py) and the GPU tests (tests/test_affine_gpu.py).

The judge: for a problem P and new affine terms a (q, r, f of every knot, g0), the ORACLE's fresh solve of P with a
substituted, and the host lqrComputeKktError on the re-solved (xs, us, vs, lbdas).

The tolerance is not fixed in advance: beside every re-solve the library's own FULL backward + forward of the
substituted problem runs on a second solver, and its distance to the oracle and its KKT triple are the yardstick.  The
re-solve may exceed the yardstick by MARGIN = 10: it applies an explicit inverse of R-hat and reuses the rounded K and
Aff, which adds a cond(R-hat) eps term to what the full solve carries.  A yardstick cannot be smaller than the rounding
of the quantity itself: the distances are floored at one eps of the solution's scale, the KKT norms at the bound
2 n eps S of kkt_device_cases.stage_residuals (two fp64 evaluations of the same residual differ by that much).
Every check prints its ratio; report() prints the largest seen (each module's docstring quotes them)."""
import ctypes as C

import numpy as np
import pytest

from aligator_amd import _lib, synth
from aligator_amd.gar import BatchedRiccatiSolver
from aligator_amd.lqr import LqrProblem, block_shapes, lqrComputeKktError
import init_stage_cases as isc
import kkt_device_cases as kc
import parity_cases as pc

EPS = kc.EPS
MARGIN = 10.0
WORST = {"distance": 0.0, "kkt": 0.0}


def report():
    print(f"affine re-solve over full solve: largest distance ratio {WORST['distance']:.3f}, "
          f"largest KKT ratio {WORST['kkt']:.3f} (margin {MARGIN:g})")


# ---- problems and affine sets ------------------------------------------------------------------------------------------
def substituted(prob, rng):
    """`prob` with new q, r, f on every knot and a new g0"""
    p = prob.copy()
    for k in p.stages:
        for name in ("q", "r", "f"):
            blk = getattr(k, name)
            blk[...] = rng.standard_normal(blk.shape)
    p.g0[...] = rng.standard_normal(p.g0.shape)
    return p


def affine_of(s, probs):
    return np.concatenate([s.pack_affine(p) for p in probs])


def resolve(s, probs):
    """upload the affine terms of `probs`, re-solve, roll out"""
    s.upload_affine(affine_of(s, probs))
    assert s.backward_affine() and s.forward()


def parts(s, b):
    """what is compared against the oracle: the solution's four parts and kkt0.ff"""
    xs, us, vs, lbdas = s.solution(b)
    return [xs, us, vs, lbdas, [s.initial(b)[0]]]


def oracle_parts(prob, mueq):
    _, osol, ref = pc.oracle_serial(prob, mueq)
    return list(ref) + [[np.array(osol.kkt0_ff, dtype=np.float64, copy=True)]]    # (a copy: the view dies with osol)


def distance(got, ref):
    return max(pc.maxdiff(A, B) for A, B in zip(got, ref)) / pc.scale_of(ref)


def kkt_floor(prob, sol, mueq):
    _, S, n = kc.stage_residuals(prob, sol, mueq)
    bound = (2.0 * n[:, None] * EPS * S).max(axis=0)
    return np.array([bound[kc.DYN], bound[kc.CST], max(bound[kc.GX], bound[kc.GU])])


def assert_resolved(s, full, probs, mueq, only=None, label=""):
    """s holds the re-solve of `probs`; `full` (same family, same batch) solves them from scratch here.  Every problem:
    distance to the oracle and host KKT triple within MARGIN of the full solve's."""
    full.upload(probs)
    assert full.backward(mueq) and full.forward()
    for b in (range(len(probs)) if only is None else only):
        ref = oracle_parts(probs[b], mueq)
        d_re, d_full = distance(parts(s, b), ref), distance(parts(full, b), ref)
        ratio = d_re / max(d_full, EPS)
        sol_re, sol_full = s.solution(b), full.solution(b)
        k_re = np.array(lqrComputeKktError(probs[b], *sol_re, mueq=mueq))
        k_full = np.array(lqrComputeKktError(probs[b], *sol_full, mueq=mueq))
        yard = np.maximum(k_full, kkt_floor(probs[b], sol_full, mueq))
        kratio = float((k_re / np.maximum(yard, 1e-300)).max())
        print(f"affine {label} b={b}: distance re-solve {d_re:.3e} full {d_full:.3e} ratio {ratio:.3f}; "
              f"kkt re-solve {k_re} full {k_full} ratio {kratio:.3f}")
        WORST["distance"], WORST["kkt"] = max(WORST["distance"], ratio), max(WORST["kkt"], kratio)
        assert np.isfinite(k_re).all() and ratio <= MARGIN and kratio <= MARGIN, (label, b, ratio, kratio)
    report()


def pair_of_solvers(probs, lib_path, **opts):
    return kc.solver_for(probs, lib_path, **opts), kc.solver_for(probs, lib_path, **opts)


def successive_sets(s, full, probs, mueq, rng, sets=3, label=""):
    """`sets` affine sets one after the other with no backward in between, then the original one again"""
    assert s.backward(mueq) and s.forward()
    for i in range(sets):
        new = [substituted(p, rng) for p in probs]
        resolve(s, new)
        assert_resolved(s, full, new, mueq, label=f"{label} set {i}")
    resolve(s, probs)
    assert_resolved(s, full, probs, mueq, label=f"{label} original")
    assert s.num_failed() == 0 and not s.status().any()


# ---- raw device records (bitwise comparisons) --------------------------------------------------------------------------
def raw_factors(s, lib_path):
    return kc.read_device(s.device_pointers()[1], s.batch * s.device_factors_doubles, lib_path).reshape(s.batch, -1)


def raw_solutions(s, lib_path):
    return kc.read_device(s.device_pointers()[2], s.batch * s.device_solution_doubles, lib_path).reshape(s.batch, -1)


def rewritten_factor_mask(s):
    """True on the entries of one problem's device factor records a re-solve may rewrite: ff and vx of every stage"""
    mask = np.zeros(s.device_factors_doubles, dtype=bool)
    for t in range(s.horizon + 1):
        nx, nu, nc, nx2, _ = (int(v) for v in s.device_dims[t])
        nr, p = nu + nc + nx2, int(s.device_stage_offsets[t, 1])
        mask[p:p + nr] = True
        vx = p + nr + nr * nx + nx * nx
        mask[vx:vx + nx] = True
    return mask


def affine_mask(s):
    """True on q, r, f of every knot and g0 inside one packed problem of the caller"""
    mask = np.zeros(s.problem_doubles, dtype=bool)
    mask[s.g0_off:s.g0_off + s.nc0] = True
    for t in range(s.horizon + 1):
        nx, nu, nc, nx2, nth = (int(v) for v in s.dims[t])
        p = int(s.stage_offsets[t, 0])
        for name, shp in block_shapes(nx, nu, nc, int(s.packed_dims[t, 3]), nth).items():
            n = int(np.prod(shp))
            if name in ("q", "r", "f"):
                mask[p:p + n] = True
            p += n
    return mask


def to_device(arr, lib_path):
    """(keep-alive object, device address) of a float64 array: host memory IS the emulator's device memory"""
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    if lib_path is not None:
        return arr, arr.ctypes.data
    import torch
    t = torch.from_numpy(arr).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr()


# ---- the cases ---------------------------------------------------------------------------------------------------------
def check_serial(lib_path, nx, nu, N, batch, kernel, mueq=1e-8, **opts):
    """case 1: a serial family, three successive affine sets with no backward between them, then the original set"""
    probs = kc.unconstrained(nx, nu, N, batch, seed=3)
    s, full = pair_of_solvers(probs, lib_path, **opts)
    assert s.kernel_name == kernel, s.kernel_name
    assert s.affine_doubles == (N + 1) * 2 * nx + N * nu + nx
    successive_sets(s, full, probs, mueq, np.random.default_rng([7, nx, nu]), label=kernel)


def check_padded(lib_path, nx, nu, N, kernel, mueq=1e-8):
    """case 2: the caller's dimensions on a padded solver; the dummy states and controls still solve to exactly zero"""
    probs = kc.unconstrained(nx, nu, N, 2, seed=4)
    s, full = pair_of_solvers(probs, lib_path, BACKWARD="wave")
    assert s.padded and s.kernel_name == kernel, (s.padded, s.kernel_name)
    successive_sets(s, full, probs, mueq, np.random.default_rng([8, nx, nu]), sets=2, label=f"padded {kernel}")
    sol = raw_solutions(s, lib_path)
    NX, NU = int(s.device_dims[0, 0]), int(s.device_dims[0, 1])
    for t in range(N + 1):
        x, u = int(s.device_stage_offsets[t, 2]), int(s.device_stage_offsets[t, 3])
        assert (sol[:, x + nx:x + NX] == 0.0).all(), t
        if t < N:
            assert (sol[:, u + nu:u + NU] == 0.0).all(), t
    assert (np.abs(sol) > 0).any()


def check_initial(lib_path, frac, kind, init, nx=8, nu=4, N=3, mueq=1e-8):
    """case 3: nc0 in {0, nx / 2, nx}, G0 = -I, +I, general, a changed g0, GAR_HIP_INIT unset and = bk"""
    nc0 = {0: 0, 1: nx // 2, 2: nx}[frac]
    rng = np.random.default_rng([9, frac, isc.G0_KINDS.index(kind)])
    probs = [isc.set_initial(p, nc0, kind, rng) for p in kc.unconstrained(nx, nu, N, 2, seed=5)]
    opts = dict(BACKWARD="wave")
    if init:
        opts["INIT"] = init
    s, full = pair_of_solvers(probs, lib_path, **opts)
    assert s.kernel_name == f"wave<{nx},{nu}>", s.kernel_name
    assert s.affine_doubles == (N + 1) * 2 * nx + N * nu + nc0
    successive_sets(s, full, probs, mueq, rng, sets=1, label=f"init nc0={nc0} G0={kind} INIT={init}")
    # g0 alone changes (through the affine vector): the sweep's records keep their bits, kkt0.ff follows the oracle
    if nc0:
        before = raw_factors(s, lib_path)
        new = [p.copy() for p in probs]
        for p in new:
            p.g0[...] += 1.0 + np.arange(nc0)
        resolve(s, new)
        assert np.array_equal(before, raw_factors(s, lib_path))
        assert_resolved(s, full, new, mueq, label="g0 alone")


def terminal_problems(which, batch=2):
    rng = np.random.default_rng([17, len(which)])
    if which == "nx2=0":          # the terminal knot as ProxDDP builds it
        nx, nu, N = 8, 4, 4
        tail = lambda: synth.generate_knot(rng, nx, 0, nx2=0, mode="W")
    elif which == "one knot":
        return kc.unconstrained(6, 3, 0, batch, seed=6)
    else:                         # a terminal knot with controls
        nx, nu, N = 6, 3, 3
        tail = lambda: synth.generate_knot(rng, nx, nu, mode="W")
    probs = []
    for _ in range(batch):
        p = LqrProblem([synth.generate_knot(rng, nx, nu, mode="W") for _ in range(N)] + [tail()], nx)
        p.G0[...] = -np.eye(nx)
        p.g0[...] = rng.standard_normal(nx)
        probs.append(p)
    return probs


def check_terminal(lib_path, which, mueq=1e-8):
    """case 4: a terminal knot with nx2 = 0 (no f in the affine vector), N = 0, a terminal knot with nu > 0"""
    probs = terminal_problems(which)
    s, full = pair_of_solvers(probs, lib_path)
    want = sum(k.nx + k.nu + k.nx2 for k in probs[0].stages) + probs[0].nc0
    assert s.affine_doubles == want, (s.affine_doubles, want)
    successive_sets(s, full, probs, mueq, np.random.default_rng(19), sets=2, label=f"terminal {which}")


def check_ring(lib_path, family, mueq=1e-8):
    """case 5: two cycleAppends (a ring: no record moves), the new knots uploaded, backward, then re-solves"""
    nx, nu, N = 8, 4, 5
    probs = kc.unconstrained(nx, nu, N, 2, seed=7)
    rng = np.random.default_rng(5)
    s, full = pair_of_solvers(probs, lib_path, BACKWARD=family)
    assert s.backward(mueq) and s.forward()
    for _ in range(2):
        s.cycle_append(probs[0].stages[0].dims)
        with pytest.raises(RuntimeError, match="gar_hip error -1.*cycle_append"):
            s.backward_affine()
        for b, p in enumerate(probs):
            new = synth.generate_knot(rng, nx, nu, mode="W")
            p.stages[:N] = p.stages[1:N] + [new]
            s.upload_knot(b, N - 1, new)
    assert int(s.stage_offsets[0, 0]) != int(s.stage_offsets[:, 0].min())      # the ring has turned
    successive_sets(s, full, probs, mueq, rng, sets=2, label=f"ring {family}")


def check_grid(lib_path, mueq=1e-8):
    """case 6: 70 problems of (8, 4), N = 3, each with its own affine vector; vector b moves problem b only; a batch of
    16 is bitwise sixteen batch-1 solvers"""
    nx, nu, N, batch = 8, 4, 3, 70
    few = kc.unconstrained(nx, nu, N, 7, seed=8)
    rng = np.random.default_rng(23)
    probs = [few[b % 7].copy() for b in range(batch)]
    s = kc.solver_for(probs, lib_path, BACKWARD="wave")
    full = kc.solver_for(probs, lib_path, BACKWARD="wave")
    assert s.backward(mueq)
    new = [substituted(p, rng) for p in probs]
    resolve(s, new)
    assert_resolved(s, full, new, mueq, only=[0, 1, 63, 64, 69], label="grid")
    base_f, base_s = raw_factors(s, lib_path), raw_solutions(s, lib_path)
    for b in (0, 63, 64, 69):
        other = substituted(new[b], rng)
        s.upload_affine(s.pack_affine(other), b)
        assert s.backward_affine() and s.forward()
        f, x = raw_factors(s, lib_path), raw_solutions(s, lib_path)
        keep = np.arange(batch) != b
        assert np.array_equal(f[keep], base_f[keep]) and np.array_equal(x[keep], base_s[keep]), b
        assert not np.array_equal(x[b], base_s[b])
        s.upload_affine(s.pack_affine(new[b]), b)
    assert s.backward_affine() and s.forward()
    assert np.array_equal(raw_factors(s, lib_path), base_f) and np.array_equal(raw_solutions(s, lib_path), base_s)
    # sixteen batch-1 solvers against one batch of sixteen
    s16 = kc.solver_for(probs[:16], lib_path, BACKWARD="wave")
    assert s16.backward(mueq)
    resolve(s16, new[:16])
    f16, x16 = raw_factors(s16, lib_path), raw_solutions(s16, lib_path)
    for b in range(16):
        s1 = kc.solver_for(probs[b:b + 1], lib_path, BACKWARD="wave")
        assert s1.kernel_name == s16.kernel_name and s1.backward(mueq)
        resolve(s1, new[b:b + 1])
        assert np.array_equal(raw_factors(s1, lib_path)[0], f16[b]), b
        assert np.array_equal(raw_solutions(s1, lib_path)[0], x16[b]), b
        assert np.array_equal(s1.initial(0)[0], s16.initial(b)[0]), b
        s1.close()


def check_untouched(lib_path, family, mueq=1e-8):
    """case 7: upload_affine moves q, r, f, g0 of the knots and nothing else; backward_affine moves ff, vx and kkt0.ff
    and nothing else of the factor records"""
    nx, nu, N = 8, 4, 4
    probs = kc.unconstrained(nx, nu, N, 3, seed=9)
    rng = np.random.default_rng(29)
    s = kc.solver_for(probs, lib_path, BACKWARD=family)
    assert s.backward(mueq) and s.forward()
    knots0, fac0 = s.download_packed().reshape(s.batch, -1), raw_factors(s, lib_path)
    fth0 = [s.initial(b)[1].copy() for b in range(s.batch)]
    new = [substituted(p, rng) for p in probs]
    s.upload_affine(affine_of(s, new))
    knots1 = s.download_packed().reshape(s.batch, -1)
    am = affine_mask(s)
    assert np.array_equal(knots0[:, ~am], knots1[:, ~am])
    want = np.concatenate([s.pack(p) for p in new]).reshape(s.batch, -1)
    assert np.array_equal(knots1[:, am], want[:, am])
    assert np.array_equal(fac0, raw_factors(s, lib_path))             # (the upload alone touches no factor)
    assert s.backward_affine()
    fac1 = raw_factors(s, lib_path)
    fm = rewritten_factor_mask(s)
    assert np.array_equal(fac0[:, ~fm], fac1[:, ~fm])
    assert not np.array_equal(fac0[:, fm], fac1[:, fm])
    for b in range(s.batch):
        assert np.array_equal(fth0[b], s.initial(b)[1])
    assert np.array_equal(knots1, s.download_packed().reshape(s.batch, -1))


def check_invalidation(lib_path, mueq=1e-8):
    """case 8: new matrices end the re-solves until the next backward; W is formed again for the new matrices"""
    nx, nu, N = 8, 4, 4
    probs = kc.unconstrained(nx, nu, N, 2, seed=10)
    others = kc.unconstrained(nx, nu, N, 2, seed=11)
    rng = np.random.default_rng(31)
    s, full = pair_of_solvers(probs, lib_path, BACKWARD="wave")
    assert s.backward(mueq)
    new = [substituted(p, rng) for p in probs]
    resolve(s, new)
    assert_resolved(s, full, new, mueq, label="before new matrices")
    fac = raw_factors(s, lib_path)
    for upload, name in ((lambda: s.upload(others), "upload_stage|upload_packed"),
                         (lambda: s.upload_knot(0, 1, others[0].stages[1]), "upload_stage")):
        upload()
        with pytest.raises(RuntimeError, match=f"gar_hip error -1.*({name})"):
            s.backward_affine()
        with pytest.raises(RuntimeError, match="gar_hip error -1"):
            s.backward_affine_async()
        assert np.array_equal(fac, raw_factors(s, lib_path))            # nothing was launched
    s.upload(others)
    assert s.backward(mueq)
    new = [substituted(p, rng) for p in others]
    resolve(s, new)
    assert_resolved(s, full, new, mueq, label="after new matrices (a stale W fails here)")
    # a backward at another mueq: the initial stage of the re-solve follows it
    probs2 = [isc.set_initial(p, nx // 2, "gen", rng) for p in others]
    s2, full2 = pair_of_solvers(probs2, lib_path, BACKWARD="wave")
    assert s2.backward(1e-3)
    new2 = [substituted(p, rng) for p in probs2]
    resolve(s2, new2)
    assert_resolved(s2, full2, new2, 1e-3, label="mueq = 1e-3")


def refused(s, lib_path, probs, mueq, sweep=True):
    if sweep:
        assert s.backward(mueq) and s.forward()
    multi = s.devices is not None
    knots = s.download_packed()
    fac = None if multi else raw_factors(s, lib_path)
    n = max(s.affine_doubles, 1)
    keep, ptr = to_device(np.ones(n * s.batch), lib_path)
    for call in (s.backward_affine, s.backward_affine_async, lambda: s.upload_affine(np.ones(n * s.batch)),
                 lambda: s.upload_affine_device(ptr)):
        with pytest.raises(RuntimeError, match="gar_hip error -3"):
            call()
    s.sync()
    assert np.array_equal(knots, s.download_packed())
    if not multi:
        assert np.array_equal(fac, raw_factors(s, lib_path))


def check_refusals(lib_path, what, devices=(0, 0), mueq=1e-6):
    """case 9: GAR_HIP_ERR_UNSUPPORTED with the knot and factor records bitwise untouched; no backward: an error"""
    nx, nu, N = 8, 4, 5
    if what == "nc":
        probs = kc.constrained(nx, nu, 2, N, 2, D=True)
        refused(kc.solver_for(probs, lib_path), lib_path, probs, mueq)
    elif what == "nth":
        rng = np.random.default_rng(37)
        probs = [synth.generate_lq_problem(rng, rng.standard_normal(nx), N, nx, nu, nth=2, mode="W", singular=False)
                 for _ in range(2)]
        refused(kc.solver_for(probs, lib_path), lib_path, probs, mueq)
    elif what == "legs":
        probs = kc.unconstrained(nx, nu, N, 2)
        refused(kc.solver_for(probs, lib_path, num_legs=2), lib_path, probs, mueq)
    elif what == "dense":
        probs = kc.unconstrained(nx, nu, N, 2)
        refused(kc.solver_for(probs, lib_path, dense=True), lib_path, probs, mueq)
    elif what == "multi":
        probs = kc.unconstrained(nx, nu, 11, 2)
        s = BatchedRiccatiSolver([k.dims for k in probs[0].stages], probs[0].nc0, batch=2, num_legs=4, lib_path=lib_path,
                                 devices=list(devices))
        s.upload(probs)
        refused(s, lib_path, probs, mueq)
    else:                                   # no backward yet
        probs = kc.unconstrained(nx, nu, N, 2)
        s = kc.solver_for(probs, lib_path)
        fac = raw_factors(s, lib_path)
        s.upload_affine(affine_of(s, probs))                    # (the upload itself needs no backward)
        for call in (s.backward_affine, s.backward_affine_async):
            with pytest.raises(RuntimeError, match="gar_hip error -1.*no backward"):
                call()
        assert np.array_equal(fac, raw_factors(s, lib_path))


def check_failed_problem(lib_path, mueq=1e-8):
    """case 10: problem 1 of three fails its backward (R-hat = 0 at knot 2); the re-solve leaves its status and factor
    records alone, solves the others, and num_failed stays 1"""
    nx, nu, N = 8, 4, 5
    probs = kc.unconstrained(nx, nu, N, 3, seed=12)
    bad = probs[1].stages[2]
    bad.R[...] = 0.0
    bad.S[...] = 0.0
    bad.B[...] = 0.0
    s, full = pair_of_solvers(probs, lib_path, BACKWARD="wave")
    pc.assert_reported_failure(s.backward, mueq)
    st = s.status()
    assert [bool(v) for v in st] == [False, True, False] and s.num_failed() == 1
    fac, init1 = raw_factors(s, lib_path), s.initial(1)[0].copy()
    rng = np.random.default_rng(41)
    new = [substituted(p, rng) for p in probs]
    s.upload_affine(affine_of(s, new))
    pc.assert_reported_failure(lambda _: s.backward_affine(), mueq)         # (reports like backward does)
    s.forward()
    after = raw_factors(s, lib_path)
    assert np.array_equal(fac[1], after[1], equal_nan=True)
    assert np.array_equal(init1, s.initial(1)[0], equal_nan=True)
    assert np.array_equal(st, s.status()) and s.num_failed() == 1
    good = [new[0], new[2]]
    full.close()
    gfull = kc.solver_for(good, lib_path, BACKWARD="wave")                  # the yardstick: the good ones on their own
    assert gfull.backward(mueq) and gfull.forward()
    for b, i in ((0, 0), (2, 1)):
        ref = oracle_parts(new[b], mueq)
        d_re, d_full = distance(parts(s, b), ref), distance(parts(gfull, i), ref)
        print(f"affine failed-batch b={b}: distance re-solve {d_re:.3e} full {d_full:.3e}")
        WORST["distance"] = max(WORST["distance"], d_re / max(d_full, EPS))
        assert d_re <= MARGIN * max(d_full, EPS), (b, d_re, d_full)
    report()


def check_allocation(lib_path, rounds=20, mueq=1e-8):
    """case 11: the first upload / re-solve may allocate; 20 further ones do not, a backward in between included"""
    L = _lib.load(lib_path)
    probs = kc.unconstrained(8, 4, 3, 3, seed=13)
    rng = np.random.default_rng(43)
    s = kc.solver_for(probs, lib_path)
    assert s.backward(mueq) and s.forward()
    c0 = L.gar_hip_debug_alloc_count()
    keep, ptr = to_device(affine_of(s, probs), lib_path)
    resolve(s, probs)
    s.upload_affine_device(ptr)
    s.backward_affine_async()
    s.sync()
    c1 = L.gar_hip_debug_alloc_count()
    assert 0 < c1 - c0 <= 4
    for i in range(rounds):
        resolve(s, [substituted(p, rng) for p in probs])
        s.upload_affine_device(ptr)
        s.backward_affine_async()
        if i == rounds // 2:
            assert s.backward(mueq)
    s.sync()
    assert L.gar_hip_debug_alloc_count() == c1


def check_no_host_sync(lib_path, mueq=1e-8, pipeline=False):
    """case 12: upload_affine_device -> backward_affine_async -> forward_async -> kkt_error_async -> sync"""
    probs = kc.unconstrained(8, 4, 5, 5, seed=14)
    rng = np.random.default_rng(47)
    s, full = pair_of_solvers(probs, lib_path, BACKWARD="wave")
    if pipeline:
        s.set_pipeline(2)
        assert s.pipeline == 2
    new = [substituted(p, rng) for p in probs]
    keep, ptr = to_device(affine_of(s, new), lib_path)
    s.backward_async(mueq)
    s.forward_async()
    for _ in range(2):
        s.upload_affine_device(ptr)
        s.backward_affine_async()
        s.forward_async()
        s.kkt_error_async(mueq)
    s.sync()
    assert s.num_failed() == 0
    err, _ = kc.device_results(s, lib_path)
    for b, p in enumerate(new):
        host = np.array(lqrComputeKktError(p, *s.solution(b), mueq=mueq))
        assert np.abs(err[b] - host).max() <= kkt_floor(p, s.solution(b), mueq).max(), b
    assert_resolved(s, full, new, mueq, label="no host sync" + (" (pipelined)" if pipeline else ""))


def check_default_batch(mueq=1e-10):
    """case 13 (GPU only): (36, 12), N = 16, batch 8 x #CUs -- the batch at which a new solver starts pipelined.
    Problems from synth_device.fill_problems, affine vectors a torch tensor on the device.  Every problem's device KKT
    triple after the re-solve within MARGIN of the triple the FULL solve of the same substituted problems gives (a
    second solver, run first); five problems spread over the batch against the host oracle."""
    import torch
    from aligator_amd import synth_device
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nx, nu, N, batch = 36, 12, 16, 8 * cus
    dims = [(nx, nu, 0, nx, 0)] * N + [(nx, 0, 0, nx, 0)]
    spread = (0, 1, batch // 2 - 1, batch // 2, batch - 1)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(53)
    full = BatchedRiccatiSolver(dims, nx, batch=batch)
    aff = torch.randn(batch, full.affine_doubles, generator=gen, device="cuda", dtype=torch.float64)
    synth_device.fill_problems(full, seed=11, mode="W")
    full.upload_affine_device(aff.data_ptr())
    full.backward_async(mueq)
    full.forward_async()
    full.kkt_error_async(mueq)
    full.sync()
    assert full.num_failed() == 0
    kkt_full = kc.device_results(full, None)[0].copy()
    d_full, refs, floors = {}, {}, {}
    for b in spread:
        p = kc.host_problem(full, b)
        refs[b] = (p, oracle_parts(p, mueq))
        d_full[b] = distance(parts(full, b), refs[b][1])
        floors[b] = kkt_floor(p, full.solution(b), mueq)
    full.close()
    s = BatchedRiccatiSolver(dims, nx, batch=batch)
    assert s.pipeline == 2 and s.kernel_name == "wave<36,12>"
    synth_device.fill_problems(s, seed=11, mode="W")             # the same matrices, the generator's own affine terms
    s.backward_async(mueq)
    s.forward_async()
    s.upload_affine_device(aff.data_ptr())
    s.backward_affine_async()
    s.forward_async()
    s.kkt_error_async(mueq)
    s.sync()
    assert s.num_failed() == 0 and not s.status().any()
    kkt_re = kc.device_results(s, None)[0]
    floor = np.max([floors[b] for b in spread], axis=0)
    kratio = float((kkt_re / np.maximum(np.maximum(kkt_full, floor), 1e-300)).max())    # (cstErr: 0 over 0)
    print(f"affine default batch: device KKT re-solve max {kkt_re.max(axis=0)} full max {kkt_full.max(axis=0)} "
          f"largest ratio {kratio:.3f}")
    WORST["kkt"] = max(WORST["kkt"], kratio)
    assert np.isfinite(kkt_re).all() and kratio <= MARGIN
    for b in spread:
        p, ref = refs[b]
        got = kc.host_problem(s, b)
        assert np.array_equal(s.pack(got), s.pack(p)), b             # the same substituted problem on both solvers
        d_re = distance(parts(s, b), ref)
        ratio = d_re / max(d_full[b], EPS)
        print(f"affine default batch b={b}: distance re-solve {d_re:.3e} full {d_full[b]:.3e} ratio {ratio:.3f}")
        WORST["distance"] = max(WORST["distance"], ratio)
        assert ratio <= MARGIN, (b, d_re, d_full[b])
    report()
    s.close()
