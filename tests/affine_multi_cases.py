"""A resident batch solved for many affine terms at once (gar_hip_affine_solve_multi, csrc/gar_affine_multi.hpp,
aligator_amd/layer.py: lq_affine_solve_multi): cases and checks shared by the emulator tests
(tests/test_affine_multi.py) and the GPU tests (tests/test_affine_multi_gpu.py).

The yardstick, per column: the dense KKT system of oracle/dense_kkt.py for the problem with (q, r, f, g0) := that column,
solved by LAPACK for all columns of a problem at once (one matrix, nrhs right-hand sides).  The bar of a column is
    max(1e-11 x the largest entry of the dense solution, 10 x the distance of the ORACLE's Riccati solve of the same
        substituted problem from the dense solution)
-- derived from the reference side alone (two independent fp64 solvers of the same system), never from the library.
Every check prints its ratio error / bar; report() prints the largest seen (each module's docstring quotes it)."""
import numpy as np
import pytest

from aligator_amd import _lib, synth
from aligator_amd.gar import BatchedRiccatiSolver
import adjoint_cases as adc
import affine_cases as ac
import init_stage_cases as isc
import kkt_device_cases as kc
import parity_cases as pc
import refine_cases as rc
from oracle import dense_kkt

WORST = {"dense": 0.0, "adjoint": 0.0}
bits = rc.bits
DevArray = adc.DevArray
NRHS = (1, 3, 16, 17, 33)       # a partial panel, a full one, a tail of one column, three panels


def report():
    print(f"affine_solve_multi over its bar against the dense KKT solve: largest ratio {WORST['dense']:.3f}; "
          f"nrhs = 1 against adjoint() over the same bar: {WORST['adjoint']:.3f}")


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
def right_hand_sides(s, nrhs, rng):
    return rng.standard_normal((s.batch, nrhs, s.affine_doubles))


def yardstick(s, prob, cols, mueq):
    """-> (dense solutions (ncols, affine_doubles), bars (ncols,)) of one problem for the affine vectors `cols`"""
    subs = [adc.with_affine(s, prob, c) for c in cols]
    mat = dense_kkt.lqr_dense_matrix(subs[0], mueq)[0]
    rhs = np.stack([dense_kkt.lqr_dense_matrix(p, mueq)[1] for p in subs], axis=1)
    Z = -np.linalg.solve(mat, rhs)
    dense = np.stack([adc.sol_to_vec(s, dense_kkt.dense_solution_to_traj(prob, Z[:, j])) for j in range(len(subs))])
    bars = np.zeros(len(subs))
    for j, p in enumerate(subs):
        riccati = adc.sol_to_vec(s, pc.oracle_serial(p, mueq)[2])
        bars[j] = max(1e-11 * float(np.abs(dense[j]).max()), 10.0 * float(np.abs(riccati - dense[j]).max()))
    return dense, bars


def yardsticks(s, probs, rhs, mueq, only=None):
    return {b: yardstick(s, probs[b], rhs[b], mueq) for b in (range(s.batch) if only is None else only)}


def assert_columns(out, ref, label="", ncols=None):
    """out (batch, nrhs, n) against the yardsticks of the problems in `ref`, its first `ncols` columns"""
    for b, (dense, bars) in ref.items():
        n = out.shape[1] if ncols is None else ncols
        assert np.isfinite(out[b, :n]).all(), (label, b)
        err = np.abs(out[b, :n] - dense[:n]).max(axis=1)
        ratio = float((err / bars[:n]).max())
        j = int(np.argmax(err / bars[:n]))
        print(f"affine_solve_multi {label} b={b}: {n} columns, worst column {j}: error {err[j]:.3e} bar {bars[j]:.3e} "
              f"ratio {ratio:.3f}, largest entry {np.abs(dense[:n]).max():.3e}")
        WORST["dense"] = max(WORST["dense"], ratio)
        assert (err <= bars[:n]).all(), (label, b, j, err[j], bars[j])
    report()


def backward_only(probs, lib_path, mueq, **opts):
    """a solver that has run its backward and NO forward: the entry point reads nothing of the primal solution"""
    s = kc.solver_for(probs, lib_path, **opts)
    assert s.backward(mueq)
    return s


def prefixes(s, probs, mueq, rng, label, nrhs_list=NRHS, only=None):
    """one set of max(nrhs_list) columns; every nrhs of the list takes its first columns (one yardstick for all)"""
    rhs = right_hand_sides(s, max(nrhs_list), rng)
    ref = yardsticks(s, probs, rhs, mueq, only)
    outs = {}
    for n in nrhs_list:
        out = s.affine_solve_multi(rhs[:, :n])
        assert out.shape == (s.batch, n, s.affine_doubles)
        assert_columns(out, ref, label=f"{label} nrhs={n}", ncols=n)
        outs[n] = out
    return rhs, ref, outs


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def check_serial(lib_path, nx, nu, N, batch, kernel, mueq=1e-10, **opts):
    """case 1: a serial family at nrhs = 1, 3, 16, 17, 33; a column's answer does not depend on how many ride with it"""
    probs = rc.singular_problems(nx, nu, N, batch)
    s = backward_only(probs, lib_path, mueq, **opts)
    assert s.kernel_name == kernel, s.kernel_name
    _, _, outs = prefixes(s, probs, mueq, np.random.default_rng([101, nx, nu]), kernel)
    for n in NRHS[:-1]:
        assert np.array_equal(bits(outs[n]), bits(outs[NRHS[-1]][:, :n])), n


def check_padded(lib_path, nx, nu, N, kernel, nrhs=5, mueq=1e-10):
    """case 2: the caller's dimensions on a padded solver: rhs and out speak them, the dummy entries appear nowhere"""
    probs = rc.singular_problems(nx, nu, N, 2)
    s = backward_only(probs, lib_path, mueq, BACKWARD="wave")
    assert s.padded and s.kernel_name == kernel, (s.padded, s.kernel_name)
    assert s.affine_doubles == (N + 1) * 2 * nx + N * nu + nx
    prefixes(s, probs, mueq, np.random.default_rng([102, nx, nu]), f"padded {kernel}", nrhs_list=(nrhs,))


def check_initial(lib_path, frac, kind, init, nx=8, nu=4, N=3, nrhs=3, mueq=1e-10):
    """case 3: nc0 in {0, nx / 2, nx}, G0 = -I, +I, general, GAR_HIP_INIT unset and = bk"""
    nc0 = {0: 0, 1: nx // 2, 2: nx}[frac]
    rng = np.random.default_rng([103, frac, isc.G0_KINDS.index(kind)])
    opts = dict(BACKWARD="wave")
    if init:
        opts["INIT"] = init
    probs = [isc.set_initial(p, nc0, kind, rng) for p in rc.singular_problems(nx, nu, N, 2)]
    s = backward_only(probs, lib_path, mueq, **opts)
    assert s.kernel_name == f"wave<{nx},{nu}>", s.kernel_name
    assert s.affine_doubles == (N + 1) * 2 * nx + N * nu + nc0
    prefixes(s, probs, mueq, rng, f"init nc0={nc0} G0={kind} INIT={init}", nrhs_list=(nrhs,))


def check_terminal(lib_path, which, nrhs=3, mueq=1e-10):
    """case 4: a terminal knot with nx2 = 0, one knot (N = 0), a terminal knot with nu > 0"""
    probs = ac.terminal_problems(which)
    s = backward_only(probs, lib_path, mueq)
    rng = np.random.default_rng(104)
    rhs, _, outs = prefixes(s, probs, mueq, rng, f"terminal {which}", nrhs_list=(nrhs,))
    slot = adc.slot_N(s)
    if slot:                     # the terminal f slot: ignored on the way in, zero on the way out
        lo = s.affine_doubles - s.nc0 - slot
        assert not outs[nrhs][:, :, lo:lo + slot].any()
        other = rhs.copy()
        other[:, :, lo:lo + slot] += 1.0
        assert np.array_equal(bits(s.affine_solve_multi(other)), bits(outs[nrhs]))


def check_ring(lib_path, family, nrhs=3, mueq=1e-10):
    """case 5: after two cycleAppends (a ring: no record moves) the panels follow the turned stage descriptors"""
    nx, nu, N = 8, 4, 5
    probs = rc.singular_problems(nx, nu, N, 2)
    rng = np.random.default_rng(105)
    s = backward_only(probs, lib_path, mueq, BACKWARD=family)
    for _ in range(2):
        s.cycle_append(probs[0].stages[0].dims)
        with pytest.raises(RuntimeError, match="gar_hip error -1.*cycle_append"):
            s.affine_solve_multi(right_hand_sides(s, nrhs, rng))
        for b, p in enumerate(probs):
            new = synth.generate_knot(rng, nx, nu, mode="F")
            p.stages[:N] = p.stages[1:N] + [new]
            s.upload_knot(b, N - 1, new)
    assert int(s.stage_offsets[0, 0]) != int(s.stage_offsets[:, 0].min())      # the ring has turned
    assert s.backward(mueq)
    prefixes(s, probs, mueq, rng, f"ring {family}", nrhs_list=(nrhs,))


def check_grid(lib_path, mueq=1e-10):
    """case 6: 70 problems of (8, 4), N = 2, 17 columns each: every (problem, column) has its own data and its own answer"""
    probs = rc.singular_problems(8, 4, 2, 70)
    s = backward_only(probs, lib_path, mueq, BACKWARD="wave")
    prefixes(s, probs, mueq, np.random.default_rng(106), "grid", nrhs_list=(17,))


def check_column_independence(lib_path, mueq=1e-10):
    """case 7: other columns, and what earlier calls left in the buffers, do not reach a column -- bit for bit"""
    nx, nu, N = 8, 4, 4
    probs = rc.singular_problems(nx, nu, N, 3)
    rng = np.random.default_rng(107)
    s = backward_only(probs, lib_path, mueq, BACKWARD="wave")
    rhs = right_hand_sides(s, 17, rng)
    out = s.affine_solve_multi(rhs)
    for j in (0, 7, 15, 16):
        other = 1e3 * right_hand_sides(s, 17, rng)
        other[:, j] = rhs[:, j]
        assert np.array_equal(bits(s.affine_solve_multi(other)[:, j]), bits(out[:, j])), j
    # a larger call with huge values, then a small one: the bits of a fresh solver (tail columns, buffers left behind)
    few = right_hand_sides(s, 3, rng)
    fresh = backward_only(probs, lib_path, mueq, BACKWARD="wave")
    want = fresh.affine_solve_multi(few)
    huge = s.affine_solve_multi(1e150 * right_hand_sides(s, 40, rng))
    assert np.isfinite(huge).all() and np.abs(huge).max() > 1e140
    assert np.array_equal(bits(s.affine_solve_multi(few)), bits(want))
    assert_columns(want, yardsticks(s, probs, few, mueq), label="after a larger call")


def check_against_adjoint(lib_path, family, mueq=1e-10):
    """case 8: nrhs = 1 against adjoint(cot)'s adj, within the column's bar (the sums are ordered differently: not bitwise)"""
    nx, nu, N = 8, 4, 5
    probs = rc.singular_problems(nx, nu, N, 3)
    s = rc.solved(probs, lib_path, mueq, BACKWARD=family)
    cot = adc.cotangents(s, np.random.default_rng(108))
    adj, _ = s.adjoint(cot, want_grad=False)
    out = s.affine_solve_multi(cot[:, None, :])
    ref = yardsticks(s, probs, cot[:, None, :], mueq)
    assert_columns(out, ref, label=f"nrhs=1 {family}")
    for b in range(s.batch):
        err, bar = float(np.abs(out[b, 0] - adj[b]).max()), float(ref[b][1][0])
        print(f"affine_solve_multi nrhs=1 {family} b={b}: against adjoint() {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
        WORST["adjoint"] = max(WORST["adjoint"], err / bar)
        assert err <= bar, (b, err, bar)
    report()


def check_untouched(lib_path, family, mueq=1e-10):
    """case 9: the call writes nothing of the primal; refine(1) and adjoint around it give the bits they give without it"""
    nx, nu, N = 8, 4, 4
    probs = rc.singular_problems(nx, nu, N, 3)
    rng = np.random.default_rng(109)
    s, plain = rc.solved(probs, lib_path, mueq, BACKWARD=family), rc.solved(probs, lib_path, mueq, BACKWARD=family)
    cot, rhs = adc.cotangents(s, rng), right_hand_sides(s, 19, rng)
    for q in (s, plain):
        assert q.refine(1) == (1, 3)                  # (W and the KKT buffers exist from here on)
    adj0, grad0 = plain.adjoint(cot)
    before = adc.snapshot(s, lib_path)
    out = s.affine_solve_multi(rhs)
    drhs, dout = DevArray(rhs.size, lib_path, rhs), DevArray(rhs.size, lib_path)
    s.affine_solve_multi_async(drhs.ptr, 19, dout.ptr)
    s.sync()
    assert np.array_equal(bits(dout.read()), bits(out.ravel()))
    after = adc.snapshot(s, lib_path)
    assert len(before) == len(after) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, after))
    adj1, grad1 = s.adjoint(cot)                      # the adjoint behind the call: the bits it gives without it
    assert np.array_equal(bits(adj0), bits(adj1)) and np.array_equal(bits(grad0), bits(grad1))
    assert np.array_equal(bits(s.affine_solve_multi(rhs)), bits(out))           # ... and the call behind the adjoint
    for q in (s, plain):
        assert q.refine(1) == (1, 3)
    assert np.array_equal(bits(ac.raw_solutions(s, lib_path)), bits(ac.raw_solutions(plain, lib_path)))
    assert np.array_equal(bits(kc.device_results(s, lib_path)[0]), bits(kc.device_results(plain, lib_path)[0]))
    assert np.array_equal(bits(s.affine_solve_multi(rhs)), bits(out))           # (the matrices have not moved)
    assert_columns(out, yardsticks(s, probs, rhs, mueq, only=(1,)), label=f"untouched {family}")


def check_failed_problem(lib_path, mueq=1e-8):
    """case 10: problem 1 of three fails its backward: exact zeros in its columns, the others within the bar"""
    nx, nu, N = 8, 4, 5
    probs = rc.singular_problems(nx, nu, N, 3)
    bad = probs[1].stages[2]
    bad.R[...] = 0.0
    bad.S[...] = 0.0
    bad.B[...] = 0.0
    s = kc.solver_for(probs, lib_path, BACKWARD="wave")
    pc.assert_reported_failure(s.backward, mueq)
    assert [bool(v) for v in s.status()] == [False, True, False]
    rhs = right_hand_sides(s, 17, np.random.default_rng(110))
    drhs, dout = DevArray(rhs.size, lib_path, rhs), DevArray(rhs.size, lib_path, np.ones(rhs.size))
    s.affine_solve_multi_async(drhs.ptr, 17, dout.ptr)             # (the asynchronous form does not wait: no report)
    s.sync()
    out = dout.read().reshape(rhs.shape)
    assert not out[1].any() and np.array_equal(bits(out[1]), bits(np.zeros_like(out[1])))
    assert_columns(out, yardsticks(s, probs, rhs, mueq, only=(0, 2)), label="failed batch")
    with pytest.raises(RuntimeError, match="Failed stage LDL factorization"):    # (the wrapper's text for GAR_HIP_ERR_FACTOR)
        s.affine_solve_multi(rhs)
    host = np.ones_like(rhs)                                       # the synchronous form's own return code and result
    PD = _lib._PD
    assert s._L.gar_hip_affine_solve_multi(s._h, 17, rhs.ctypes.data_as(PD), host.ctypes.data_as(PD)) == -4
    assert np.array_equal(bits(host), bits(out))
    assert [bool(v) for v in s.status()] == [False, True, False] and s.num_failed() == 1


class _Host:
    """two host arrays for the synchronous form called on the C ABI directly (dimensions the Python wrapper would refuse)"""

    def __init__(self, n):
        self.a, self.b = np.ones(n), np.zeros(n)


def c_forms(s, lib_path, nrhs=3):
    """the synchronous form on host arrays and the asynchronous one on device arrays, through the C ABI"""
    n = s.batch * max(nrhs, 1) * max(s.affine_doubles, 1)
    h = _Host(n)
    drhs, dout = DevArray(n, lib_path, np.ones(n)), DevArray(n, lib_path)
    PD = _lib._PD

    def sync_form():
        try:
            s._check(s._L.gar_hip_affine_solve_multi(s._h, nrhs, h.a.ctypes.data_as(PD), h.b.ctypes.data_as(PD)))
        finally:
            assert not h.b.any()

    def async_form():
        try:
            s.affine_solve_multi_async(drhs.ptr, nrhs, dout.ptr)
        finally:
            s.sync()
            assert not dout.read().any()                               # nothing written
    return sync_form, async_form


def check_refusals(lib_path, what, devices=(0, 0), mueq=1e-6):
    """case 11: the unserved kinds answer GAR_HIP_ERR_UNSUPPORTED; no backward, new matrices, nrhs = 0 and null pointers
    GAR_HIP_ERR_ARG -- with everything untouched; after new matrices the next backward serves again"""
    nx, nu, N = 8, 4, 5
    if what == "nc":
        s = rc.solved(kc.constrained(nx, nu, 2, N, 2, D=True), lib_path, mueq)
    elif what == "nth":
        rng = np.random.default_rng(37)
        probs = [synth.generate_lq_problem(rng, rng.standard_normal(nx), N, nx, nu, nth=2, mode="W", singular=False)
                 for _ in range(2)]
        s = rc.solved(probs, lib_path, mueq)
    elif what == "legs":
        s = rc.solved(kc.unconstrained(nx, nu, N, 2), lib_path, mueq, num_legs=2)
    elif what == "dense":
        s = rc.solved(kc.unconstrained(nx, nu, N, 2), lib_path, mueq, dense=True)
    elif what == "multi":
        probs = kc.unconstrained(nx, nu, 11, 2)
        s = BatchedRiccatiSolver([k.dims for k in probs[0].stages], probs[0].nc0, batch=2, num_legs=4, lib_path=lib_path,
                                 devices=list(devices))
        s.upload(probs)
        assert s.backward(mueq) and s.forward()
    elif what == "no backward":
        s = kc.solver_for(kc.unconstrained(nx, nu, N, 2), lib_path)
        return rc.untouched_by(s, lib_path, c_forms(s, lib_path), -1, "no backward")
    elif what == "new matrices":
        probs, others = rc.singular_problems(nx, nu, N, 2), kc.unconstrained(nx, nu, N, 2, seed=11)
        s = rc.solved(probs, lib_path, mueq)
        rng = np.random.default_rng(111)
        prefixes(s, probs, mueq, rng, "before new matrices", nrhs_list=(3,))
        s.upload(others)
        rc.untouched_by(s, lib_path, c_forms(s, lib_path), -1, r"\(gar_hip_upload_stage|gar_hip_upload_packed\)")
        assert s.backward(mueq)
        prefixes(s, others, mueq, rng, "after new matrices (a stale W fails here)", nrhs_list=(3,))
        return
    elif what == "nrhs = 0":
        s = rc.solved(kc.unconstrained(nx, nu, N, 2), lib_path, mueq)
        return rc.untouched_by(s, lib_path, c_forms(s, lib_path, nrhs=0) + c_forms(s, lib_path, nrhs=-2), -1, "nrhs")
    else:                                   # null pointers
        s = rc.solved(kc.unconstrained(nx, nu, N, 2), lib_path, mueq)
        d = DevArray(2 * 3 * s.affine_doubles, lib_path)
        h = np.zeros(2 * 3 * s.affine_doubles)
        PD = _lib._PD
        calls = (lambda: s._check(s._L.gar_hip_affine_solve_multi(s._h, 3, None, h.ctypes.data_as(PD))),
                 lambda: s._check(s._L.gar_hip_affine_solve_multi(s._h, 3, h.ctypes.data_as(PD), None)),
                 lambda: s.affine_solve_multi_async(0, 3, d.ptr), lambda: s.affine_solve_multi_async(d.ptr, 3, 0))
        rc.untouched_by(s, lib_path, calls, -1, "null")
        s.sync()
        assert not d.read().any() and not h.any()
        return
    rc.untouched_by(s, lib_path, c_forms(s, lib_path), -3)


def check_allocation(lib_path, rounds=20, mueq=1e-10):
    """case 12: the first calls may allocate; twenty further rounds, nrhs going through 1, 40, 16 and the two forms taking
    turns, do not -- a backward, a refine and an adjoint in between included"""
    L = _lib.load(lib_path)
    probs = rc.singular_problems(8, 4, 2, 2)
    s = rc.solved(probs, lib_path, mueq)
    assert s.refine(1) == (1, 2)
    rng = np.random.default_rng(112)
    cot = adc.cotangents(s, rng)
    s.adjoint(cot)                       # (the re-solve's, the refinement's and the adjoint's buffers exist from here on)
    sets = {n: right_hand_sides(s, n, rng) for n in (1, 40, 16)}
    dev = {n: (DevArray(r.size, lib_path, r), DevArray(r.size, lib_path)) for n, r in sets.items()}
    c0 = L.gar_hip_debug_alloc_count()
    first = s.affine_solve_multi(sets[1])
    s.affine_solve_multi_async(dev[1][0].ptr, 1, dev[1][1].ptr)
    s.sync()
    c1 = L.gar_hip_debug_alloc_count()
    assert 0 < c1 - c0 <= 7             # five work buffers and the gate words (6), the host form's staging (1)
    assert np.array_equal(bits(dev[1][1].read()), bits(first.ravel()))
    results = {}
    for i in range(rounds):
        n = (1, 40, 16)[i % 3]
        if i % 2:
            out = s.affine_solve_multi(sets[n]).ravel()
        else:
            s.affine_solve_multi_async(dev[n][0].ptr, n, dev[n][1].ptr)
            s.sync()
            out = dev[n][1].read()
        assert np.array_equal(bits(results.setdefault(n, out)), bits(out)), (i, n)     # (either form, every round: the same bits)
        if i == rounds // 2:
            assert s.backward(mueq) and s.forward() and s.refine(1) == (1, 2)
            s.adjoint(cot)
    assert L.gar_hip_debug_alloc_count() == c1
    assert np.array_equal(bits(s.affine_solve_multi(sets[1])), bits(first))
    assert_columns(results[40].reshape(sets[40].shape), yardsticks(s, probs, sets[40], mueq, only=(1,)), label="allocation nrhs=40")


def same_solutions(s, other, label):
    for b in range(s.batch):
        for part, want in zip(s.solution(b), other.solution(b)):
            assert len(part) == len(want) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(part, want)), (label, b)


def check_rebuild_with_services_live(lib_path, mueq=1e-10):
    """case 15: two cycleAppends that change the dimensions while the work areas of every resident-batch service are live:
    they go with the layout, and what the next calls build serves the new dimensions -- the bits of a fresh solver"""
    nx, nu, N = 8, 4, 3
    probs = rc.singular_problems(nx, nu, N, 2)
    rng = np.random.default_rng(115)
    s = rc.solved(probs, lib_path, mueq, BACKWARD="wave")
    s.kkt_error(mueq)
    assert s.refine(1) == (1, 2)
    s.adjoint(adc.cotangents(s, rng))
    s.affine_solve_multi(right_hand_sides(s, 17, rng))
    ac.resolve(s, [ac.substituted(p, rng) for p in probs])
    assert s.affine_doubles == (N + 1) * 2 * nx + N * nu + nx == 84
    assert all(s.device_kkt_errors()) and s.device_adjoints()
    for nu_new, doubles in ((5, 85), (3, 84)):
        s.cycle_append((nx, nu_new, 0, nx, 0))
        assert s.device_kkt_errors() == (None, None) and not s.device_adjoints()
        new = []
        for p in probs:
            q = p.copy()
            q.stages[:N] = q.stages[1:N] + [synth.generate_knot(rng, nx, nu_new, 0, mode="W")]
            new.append(q)
        probs = new
        s.upload(probs)
        fresh = kc.solver_for(probs, lib_path)
        assert s.kernel_name == fresh.kernel_name == "generic", (s.kernel_name, fresh.kernel_name)
        assert s.affine_doubles == fresh.affine_doubles == doubles
        for q in (s, fresh):
            assert q.backward(mueq) and q.forward()
        label = f"rebuilt, appended nu={nu_new}"
        rhs = right_hand_sides(s, 17, rng)
        out = s.affine_solve_multi(rhs)
        assert np.array_equal(bits(out), bits(fresh.affine_solve_multi(rhs))), label
        assert_columns(out, yardsticks(s, probs, rhs, mueq), label=label)
        cot = adc.cotangents(s, rng)
        for a, b in zip(s.adjoint(cot), fresh.adjoint(cot)):
            assert np.array_equal(bits(a), bits(b)), label
        assert s.refine(1) == fresh.refine(1), label
        same_solutions(s, fresh, label)
        others = [ac.substituted(p, rng) for p in probs]
        for q in (s, fresh):
            ac.resolve(q, others)
        same_solutions(s, fresh, label)
        assert np.array_equal(s.kkt_error(mueq), fresh.kkt_error(mueq)), label


def check_no_host_sync(lib_path, mueq=1e-10, pipeline=False, nrhs=19):
    """case 13: upload_packed_user_device -> backward_async -> affine_solve_multi_async -> sync with no host wait in
    between: bitwise what the synchronous calls give (adjoint_cases.check_no_host_sync's check)"""
    probs = rc.singular_problems(8, 4, 5, 5)
    s, ref = kc.solver_for(probs, lib_path, BACKWARD="wave"), kc.solver_for(probs, lib_path, BACKWARD="wave")
    if pipeline:
        for q in (s, ref):
            q.set_pipeline(2)
            assert q.pipeline == 2
    rhs = right_hand_sides(s, nrhs, np.random.default_rng(113))
    packed = np.concatenate([s.pack(p) for p in probs])
    src, drhs, dout = DevArray(packed.size, lib_path, packed), DevArray(rhs.size, lib_path, rhs), DevArray(rhs.size, lib_path)
    s.upload_packed_user_device(src.ptr)
    s.backward_async(mueq)
    s.affine_solve_multi_async(drhs.ptr, nrhs, dout.ptr)
    s.forward_async()
    s.sync()
    assert s.num_failed() == 0
    assert ref.backward(mueq)
    want = ref.affine_solve_multi(rhs)
    assert np.array_equal(bits(dout.read()), bits(want.ravel()))
    assert_columns(want, yardsticks(s, probs, rhs, mueq), label="no host sync" + (" (pipelined)" if pipeline else ""))


def check_layer(lib_path, device, mueq=1e-10):
    """case 14: lq_affine_solve_multi on (8, 4), N = 5, batch 3, nrhs = 17 against the yardstick; the bits of the array form"""
    import torch
    from aligator_amd.layer import lq_affine_solve_multi
    probs = rc.singular_problems(8, 4, 5, 3)
    s = backward_only(probs, lib_path, mueq, BACKWARD="wave")
    rhs = right_hand_sides(s, 17, np.random.default_rng(114))
    t = torch.tensor(rhs, dtype=torch.float64, device=device)
    out = lq_affine_solve_multi(s, t)
    if device != "cpu":
        torch.cuda.synchronize()
    s.sync()
    assert out.shape == t.shape and out.device == t.device
    got = out.cpu().numpy()
    assert_columns(got, yardsticks(s, probs, rhs, mueq), label=f"layer on {device}")
    assert np.array_equal(bits(got), bits(s.affine_solve_multi(rhs)))
    with pytest.raises(ValueError, match="rhs must be float64"):
        lq_affine_solve_multi(s, t[:, :, :-1])
