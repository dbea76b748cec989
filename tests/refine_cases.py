"""Iterative refinement of a resident batch from the stored factorisation (gar_hip_refine, csrc/gar_refine.hpp, DESIGN.md
5.3d): cases and checks shared by the emulator tests (tests/test_refine.py) and the GPU tests (tests/test_refine_gpu.py).

The yardstick is the reference, not the code under test.  For a problem and the solution z0 the library holds, the host
forms the KKT residual vectors in numpy (residual_vectors: term by term kkt_device_cases.stage_residuals, which keeps only
their norms), solves the correction problem -- the same matrices, the residuals as q, r, f, g0 -- with the ORACLE's
ProximalRiccatiSolver and evaluates lqrComputeKktError(z0 + delta).  The device's triple after one step may exceed
max(that, affine_cases.kkt_floor) by affine_cases.MARGIN = 10: the project's margin for an explicit inverse of R-hat and
the stored, rounded K and Aff; the floor is the 2 n eps S bound of DESIGN.md 5.3b.  Solutions are compared by their
distance to the oracle's full solve: after a step at most MARGIN x max(the distance before the step, eps).
At (8, 4), and at (36, 12) with N = 4, the first solve already sits at that floor and the correction is rounding-sized: a
wrong term of it would hide under the floor.  So every family, record format and initial-stage kind ALSO takes a step
whose residual is O(1) (step_from_afar): new q, r, f, g0 without a re-solve, one step, and the result within MARGIN of
where the library's own full solve of the substituted problem lands.
Every check prints its ratio; report() prints the largest seen (each module's docstring quotes them)."""
import numpy as np
import pytest

from aligator_amd import _lib, synth
from aligator_amd.gar import BatchedRiccatiSolver
from aligator_amd.lqr import lqrComputeKktError
import affine_cases as ac
import init_stage_cases as isc
import kkt_device_cases as kc
import parity_cases as pc

EPS = kc.EPS
MARGIN = ac.MARGIN
WORST = {"kkt": 0.0, "distance": 0.0, "afar_kkt": 0.0, "afar_distance": 0.0}


def report():
    print(f"refinement step over the oracle's step: largest KKT ratio {WORST['kkt']:.3f}, "
          f"largest distance ratio {WORST['distance']:.3f}; a step from an O(1) residual over the full solve: KKT "
          f"{WORST['afar_kkt']:.3f}, distance {WORST['afar_distance']:.3f} (margin {MARGIN:g})")


# ---- the yardstick -----------------------------------------------------------------------------------------------------
def residual_vectors(prob, sol):
    """-> ([gx_t], [gu_t], [dyn_t], g0 + G0 x0) of an unconstrained problem (utils.hxx:116-178), plain fp64"""
    xs, us, _, lbdas = sol
    N = prob.horizon
    gxs, gus, dyns = [], [], []
    for t, k in enumerate(prob.stages):
        x = xs[t]
        u = us[t] if k.nu > 0 else np.zeros(0)
        gx = k.q + k.Q @ x
        gu = k.r + k.S.T @ x
        if k.nu > 0:
            gx = gx + k.S @ u
            gu = gu + k.R @ u
        gx = gx + prob.G0.T @ lbdas[0] if t == 0 else gx - lbdas[t]
        dyn = np.zeros(k.f.shape)
        if t < N:
            dyn = k.A @ x + k.B @ u + k.f - xs[t + 1]
            gx = gx + k.A.T @ lbdas[t + 1]
            gu = gu + k.B.T @ lbdas[t + 1]
        gxs.append(gx), gus.append(gu), dyns.append(dyn)
    return gxs, gus, dyns, prob.g0 + prob.G0 @ xs[0]


def oracle_step(prob, z0, mueq):
    """z0 + delta, delta the oracle's solution of the correction problem"""
    gxs, gus, dyns, ini = residual_vectors(prob, z0)
    cp = prob.copy()
    for k, gx, gu, dyn in zip(cp.stages, gxs, gus, dyns):
        k.q[...], k.r[...], k.f[...] = gx, gu, dyn
    cp.g0[...] = ini
    delta = pc.oracle_serial(cp, mueq)[2]
    return tuple([a + d for a, d in zip(A, D)] for A, D in zip(z0, delta))


def triple(prob, sol, mueq):
    return np.array(lqrComputeKktError(prob, *sol, mueq=mueq))


def err_of(kkt):
    """the gate's quantity: max(dynErr, dualErr)"""
    return np.maximum(kkt[..., 0], kkt[..., 2])


def solutions(s, only=None):
    return {b: s.solution(b) for b in (range(s.batch) if only is None else only)}


def assert_step(s, probs, z0s, mueq, lib_path, label=""):
    """s has taken one step from the solutions z0s (problem -> solution): the device's triple within MARGIN of the
    yardstick's, the distance to the oracle's full solve within MARGIN of the distance before the step"""
    dev = kc.device_results(s, lib_path)[0]
    for b, z0 in z0s.items():
        z1 = oracle_step(probs[b], z0, mueq)
        yard = np.maximum(triple(probs[b], z1, mueq), ac.kkt_floor(probs[b], z1, mueq))
        kratio = float((dev[b] / np.maximum(yard, 1e-300)).max())
        ref = pc.oracle_serial(probs[b], mueq)[2]
        d0, d1 = ac.distance(z0, ref), ac.distance(s.solution(b), ref)
        dratio = d1 / max(d0, EPS)
        print(f"refine {label} b={b}: device {dev[b]} before {triple(probs[b], z0, mueq)} yardstick {yard} "
              f"ratio {kratio:.3f}; distance {d1:.3e} before {d0:.3e} ratio {dratio:.3f}")
        WORST["kkt"], WORST["distance"] = max(WORST["kkt"], kratio), max(WORST["distance"], dratio)
        assert np.isfinite(dev[b]).all() and kratio <= MARGIN and dratio <= MARGIN, (label, b, kratio, dratio)
        host = triple(probs[b], s.solution(b), mueq)           # the buffers describe the solution that is in HBM
        assert np.abs(dev[b] - host).max() <= ac.kkt_floor(probs[b], s.solution(b), mueq).max(), (label, b)
    report()


def steps_against_yardstick(s, probs, mueq, lib_path, steps=2, only=None, label=""):
    for i in range(steps):
        z0s = solutions(s, only)
        assert s.refine(1) == (1, s.batch)
        assert_step(s, probs, z0s, mueq, lib_path, label=f"{label} step {i + 1}")
    assert s.num_failed() == 0 and not s.status().any()


def step_from_afar(s, probs, mueq, lib_path, rng, only=None, label="", **opts):
    """A step whose residual is O(1): new q, r, f, g0 are uploaded with NO re-solve and no forward, so rho is the residual
    of the old solution against the new affine terms and delta is as large as the solutions themselves -- a wrong term of
    the sweep, the initial stage or the roll-out shows at that size, not at rounding.  One step must land where the
    library's own full solve of the substituted problems lands (a second solver, same family): distance to the oracle's
    full solve and device KKT triple within MARGIN of the full solve's (ac.assert_resolved's yardstick, without kkt0.ff,
    which a refinement does not write).  -> the substituted problems, which s now holds."""
    new = [ac.substituted(p, rng) for p in probs]
    if opts.pop("enqueued", False):                # upload_affine_device -> refine_async, no host wait between them
        keep, ptr = ac.to_device(ac.affine_of(s, new), lib_path)
        s.upload_affine_device(ptr)
        s.refine_async(1)
        s.sync()
    else:
        s.upload_affine(ac.affine_of(s, new))
        assert s.refine(1) == (1, s.batch)
    dev = kc.device_results(s, lib_path)[0]
    full = solved(new, lib_path, mueq, **opts)
    assert full.kernel_name == s.kernel_name
    for b in (range(s.batch) if only is None else only):
        ref = pc.oracle_serial(new[b], mueq)[2]
        sol_full = full.solution(b)
        d_re, d_full = ac.distance(s.solution(b), ref), ac.distance(sol_full, ref)
        dratio = d_re / max(d_full, EPS)
        yard = np.maximum(triple(new[b], sol_full, mueq), ac.kkt_floor(new[b], sol_full, mueq))
        kratio = float((dev[b] / np.maximum(yard, 1e-300)).max())
        print(f"refine {label} from afar b={b}: distance {d_re:.3e} full solve {d_full:.3e} ratio {dratio:.3f}; "
              f"device {dev[b]} full solve's yardstick {yard} ratio {kratio:.3f}")
        WORST["afar_distance"], WORST["afar_kkt"] = max(WORST["afar_distance"], dratio), max(WORST["afar_kkt"], kratio)
        assert np.isfinite(dev[b]).all() and dratio <= MARGIN and kratio <= MARGIN, (label, b, dratio, kratio)
    full.close()
    report()
    return new


def singular_problems(nx, nu, N, batch):
    """the reference's riccati_random_large_problem recipe: A uniform in [-1, 1], a singular Q (mode "F")"""
    return [synth.generate_lq_problem(np.random.default_rng(seed), np.ones(nx), N, nx, nu, singular=True, mode="F")
            for seed in range(batch)]


def solved(probs, lib_path, mueq, **opts):
    s = kc.solver_for(probs, lib_path, **opts)
    assert s.backward(mueq) and s.forward()
    return s


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def raw_knots(s, lib_path):
    return kc.read_device(s.device_pointers()[0], s.batch * s.device_problem_doubles, lib_path).reshape(s.batch, -1)


# ---- the cases ---------------------------------------------------------------------------------------------------------
def check_serial(lib_path, nx, nu, N, batch, kernel, mueq=1e-10, **opts):
    """case 1: a serial family, one step and then a second, each against the yardstick"""
    probs = singular_problems(nx, nu, N, batch)
    s = solved(probs, lib_path, mueq, **opts)
    assert s.kernel_name == kernel, s.kernel_name
    steps_against_yardstick(s, probs, mueq, lib_path, label=kernel)
    step_from_afar(s, probs, mueq, lib_path, np.random.default_rng([71, nx, nu]), label=kernel, **opts)


def check_improves(lib_path, mueq=1e-10):
    """case 2: (36, 12), N = 20, seeds 0-2: where the oracle's step gains two digits of dualErr, the device's gains one"""
    nx, nu, N = 36, 12, 20
    probs = singular_problems(nx, nu, N, 3)
    s = solved(probs, lib_path, mueq, BACKWARD="wave")
    assert s.kernel_name == "wave<36,12>"
    before = s.kkt_error(mueq)
    z0s = solutions(s)
    for b, z0 in z0s.items():       # a precondition on the inputs: there is something to improve
        k0, k1 = triple(probs[b], z0, mueq), triple(probs[b], oracle_step(probs[b], z0, mueq), mueq)
        print(f"refine improves b={b}: host dualErr {k0[2]:.3e} -> {k1[2]:.3e} by the oracle's step ({k0[2] / k1[2]:.0f} x)")
        assert k1[2] * 100.0 <= k0[2], (b, k0, k1)
    assert s.refine(1) == (1, 3)
    after = kc.device_results(s, lib_path)[0]
    for b in range(3):
        floor = ac.kkt_floor(probs[b], s.solution(b), mueq)
        print(f"refine improves b={b}: device dualErr {before[b, 2]:.3e} -> {after[b, 2]:.3e} "
              f"({before[b, 2] / after[b, 2]:.0f} x), dynErr {before[b, 0]:.3e} -> {after[b, 0]:.3e}")
        assert after[b, 2] <= before[b, 2] / 10.0, (b, before[b], after[b])
        assert after[b, 0] <= max(before[b, 0], floor[0] * MARGIN), (b, before[b], after[b])
    assert_step(s, probs, z0s, mueq, lib_path, label="improves")


def check_padded(lib_path, nx, nu, N, kernel, mueq=1e-10):
    """case 3: the caller's dimensions on a padded solver; the dummy states and controls stay exactly zero"""
    probs = singular_problems(nx, nu, N, 2)
    s = solved(probs, lib_path, mueq, BACKWARD="wave")
    assert s.padded and s.kernel_name == kernel, (s.padded, s.kernel_name)
    steps_against_yardstick(s, probs, mueq, lib_path, label=f"padded {kernel}")
    step_from_afar(s, probs, mueq, lib_path, np.random.default_rng([72, nx, nu]), label=f"padded {kernel}", BACKWARD="wave")
    sol = ac.raw_solutions(s, lib_path)
    NX, NU = int(s.device_dims[0, 0]), int(s.device_dims[0, 1])
    for t in range(N + 1):
        x, u = int(s.device_stage_offsets[t, 2]), int(s.device_stage_offsets[t, 3])
        assert (sol[:, x + nx:x + NX] == 0.0).all(), t
        if t < N:
            assert (sol[:, u + nu:u + NU] == 0.0).all(), t
    assert (np.abs(sol) > 0).any()


def check_initial(lib_path, frac, kind, init, nx=8, nu=4, N=3, mueq=1e-10):
    """case 4: nc0 in {0, nx / 2, nx}, G0 = -I, +I, general, GAR_HIP_INIT unset and = bk"""
    nc0 = {0: 0, 1: nx // 2, 2: nx}[frac]
    rng = np.random.default_rng([9, frac, isc.G0_KINDS.index(kind)])
    probs = [isc.set_initial(p, nc0, kind, rng) for p in singular_problems(nx, nu, N, 2)]
    opts = dict(BACKWARD="wave")
    if init:
        opts["INIT"] = init
    s = solved(probs, lib_path, mueq, **opts)
    assert s.kernel_name == f"wave<{nx},{nu}>", s.kernel_name
    init0 = [s.initial(b)[0].copy() for b in range(2)]
    steps_against_yardstick(s, probs, mueq, lib_path, label=f"init nc0={nc0} G0={kind} INIT={init}")
    step_from_afar(s, probs, mueq, lib_path, rng, label=f"init nc0={nc0} G0={kind} INIT={init}", **opts)
    for b in range(2):
        assert np.array_equal(init0[b], s.initial(b)[0])         # kkt0.ff of the factor record is not written


def check_terminal(lib_path, which, mueq=1e-10):
    """case 5: a terminal knot with nx2 = 0, one knot (N = 0), a terminal knot with nu > 0"""
    probs = ac.terminal_problems(which)
    s = solved(probs, lib_path, mueq)
    steps_against_yardstick(s, probs, mueq, lib_path, label=f"terminal {which}")
    step_from_afar(s, probs, mueq, lib_path, np.random.default_rng(73), label=f"terminal {which}")


def check_ring(lib_path, family, mueq=1e-10):
    """case 6: two cycleAppends (a ring: no record moves), the new knots uploaded, backward, forward, refine"""
    nx, nu, N = 8, 4, 5
    probs = singular_problems(nx, nu, N, 2)
    rng = np.random.default_rng(5)
    s = solved(probs, lib_path, mueq, BACKWARD=family)
    for _ in range(2):
        s.cycle_append(probs[0].stages[0].dims)
        with pytest.raises(RuntimeError, match="gar_hip error -1.*cycle_append"):
            s.refine(1)
        for b, p in enumerate(probs):
            new = synth.generate_knot(rng, nx, nu, mode="F")
            p.stages[:N] = p.stages[1:N] + [new]
            s.upload_knot(b, N - 1, new)
    assert int(s.stage_offsets[0, 0]) != int(s.stage_offsets[:, 0].min())      # the ring has turned
    assert s.backward(mueq) and s.forward()
    steps_against_yardstick(s, probs, mueq, lib_path, label=f"ring {family}")
    step_from_afar(s, probs, mueq, lib_path, rng, label=f"ring {family}", BACKWARD=family)


def check_grid(lib_path, mueq=1e-10):
    """case 7: 70 problems of (8, 4), N = 2, each with its own data, each against its own yardstick"""
    probs = singular_problems(8, 4, 2, 70)
    s = solved(probs, lib_path, mueq, BACKWARD="wave")
    steps_against_yardstick(s, probs, mueq, lib_path, steps=1, label="grid")
    step_from_afar(s, probs, mueq, lib_path, np.random.default_rng(74), label="grid", BACKWARD="wave")


def gains_and_values(s):
    s._factors_cache = {}
    out = []
    for b in range(s.batch):
        for t in range(s.horizon + 1):
            f = s.factor(t, b)
            out += [f.ff.copy(), f.fb.copy(), f.vm.Vxx.copy(), f.vm.vx.copy()]
        out.append(s.initial(b)[0].copy())
    s._factors_cache = {}
    return out


def check_untouched(lib_path, family, mueq=1e-10):
    """case 8: refine moves the solution records and the KKT buffers and nothing else"""
    nx, nu, N = 8, 4, 4
    probs = singular_problems(nx, nu, N, 3)
    rng = np.random.default_rng(29)
    new = [ac.substituted(p, rng) for p in probs]
    s = solved(probs, lib_path, mueq, BACKWARD=family)
    knots0, packed0, fac0 = raw_knots(s, lib_path), s.download_packed(), ac.raw_factors(s, lib_path)
    gv0, st0, sol0 = gains_and_values(s), s.status(), ac.raw_solutions(s, lib_path)
    assert s.refine(2) == (2, 3)
    s.refine_async(1)
    s.sync()
    assert np.array_equal(bits(knots0), bits(raw_knots(s, lib_path))) and np.array_equal(bits(packed0), bits(s.download_packed()))
    assert np.array_equal(bits(fac0), bits(ac.raw_factors(s, lib_path)))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(gv0, gains_and_values(s)))
    assert np.array_equal(st0, s.status())
    assert not np.array_equal(sol0, ac.raw_solutions(s, lib_path))
    # a re-solve after a refine gives bitwise what it gives without the refine
    plain = solved(probs, lib_path, mueq, BACKWARD=family)
    for q in (s, plain):
        ac.resolve(q, new)
    assert np.array_equal(bits(ac.raw_factors(s, lib_path)), bits(ac.raw_factors(plain, lib_path)))
    assert np.array_equal(bits(ac.raw_solutions(s, lib_path)), bits(ac.raw_solutions(plain, lib_path)))
    for b in range(3):
        assert np.array_equal(s.initial(b)[0], plain.initial(b)[0])


def gate_problems():
    """three problems whose first-solve errors lie far apart: case 2's (a step gains two digits there), the affine terms
    of the outer two scaled down -- their solutions and every residual scale with them"""
    probs = singular_problems(36, 12, 20, 3)
    for p in (probs[0], probs[2]):
        for k in p.stages:
            for name in ("q", "r", "f"):
                getattr(k, name)[...] *= 1e-4
        p.g0[...] *= 1e-4
    return probs


def check_gate(lib_path, mueq=1e-10):
    """case 9: the threshold gates on the device; a non-finite problem is skipped"""
    probs = gate_problems()
    s = solved(probs, lib_path, mueq, BACKWARD="wave")
    e = err_of(s.kkt_error(mueq))
    order = np.argsort(e)
    top, nxt = int(order[2]), int(order[1])
    print(f"refine gate: first-solve errors {e}")
    thr = float(e[top]) / 8.0
    # preconditions on the inputs: room for a threshold, and the ORACLE's step brings the top problem below it with the
    # margin to spare -- so a device step that meets the yardstick suffices
    k1 = triple(probs[top], oracle_step(probs[top], s.solution(top), mueq), mueq)
    print(f"refine gate: threshold {thr:.3e}, the oracle's step on problem {top} reaches {err_of(k1):.3e}")
    assert top == 1 and e[nxt] * 8.0 < thr and err_of(k1) * MARGIN <= thr
    sol0 = ac.raw_solutions(s, lib_path)
    s.refine_async(1, thr)
    s.sync()
    sol1 = ac.raw_solutions(s, lib_path)
    for b in range(3):
        assert np.array_equal(bits(sol0[b]), bits(sol1[b])) == (b != top), b
    # the synchronous form stops as soon as nobody is above the threshold
    s2 = solved(probs, lib_path, mueq, BACKWARD="wave")
    steps, remaining = s2.refine(5, thr)
    e2 = err_of(kc.device_results(s2, lib_path)[0])
    print(f"refine gate: threshold {thr:.3e}: {steps} step(s), {remaining} above, errors {e2}")
    assert remaining == 0 and 1 <= steps < 5 and (e2 <= thr).all()
    assert steps == 1                                  # (one step suffices here: the oracle's step gains two digits)
    assert np.array_equal(bits(ac.raw_solutions(s2, lib_path)), bits(sol1))
    assert s2.refine(5, float(e.max()) * 2.0) == (0, 0)            # nobody above: no step
    # threshold < 0 refines all
    s3 = solved(probs, lib_path, mueq, BACKWARD="wave")
    assert s3.refine(1, -1.0) == (1, 3)
    sol3 = ac.raw_solutions(s3, lib_path)
    assert all(not np.array_equal(bits(sol0[b]), bits(sol3[b])) for b in range(3))
    # a problem whose solution is NaN is skipped and stays as it is
    bad = [p.copy() for p in probs]
    bad[1].stages[2].q[0] = np.nan
    s3.upload_affine(ac.affine_of(s3, bad))
    assert s3.backward_affine() and s3.forward()
    sol4 = ac.raw_solutions(s3, lib_path)
    assert np.isnan(sol4[1]).any() and np.isfinite(sol4[[0, 2]]).all()
    assert s3.refine(3, -1.0) == (3, 2)
    sol5 = ac.raw_solutions(s3, lib_path)
    assert np.array_equal(bits(sol4[1]), bits(sol5[1]))
    assert not np.array_equal(bits(sol4[0]), bits(sol5[0])) and not np.array_equal(bits(sol4[2]), bits(sol5[2]))
    assert not np.isfinite(kc.device_results(s3, lib_path)[0][1]).all()


def check_kkt_buffers(lib_path, mueq=1e-8):
    """case 10: after either form the KKT buffers equal, bitwise, what a following kkt_error_async writes"""
    probs = singular_problems(8, 4, 4, 3)
    s = solved(probs, lib_path, mueq, BACKWARD="wave")
    for call in (lambda: s.refine(1), lambda: s.refine_async(2), lambda: s.refine(0), lambda: s.refine_async(0),
                 lambda: s.refine(3, 1.0)):
        call()
        s.sync()
        err, st = kc.device_results(s, lib_path)
        s.kkt_error_async(mueq)
        s.sync()
        err2, st2 = kc.device_results(s, lib_path)
        assert np.array_equal(bits(err), bits(err2)) and np.array_equal(bits(st), bits(st2))
        assert np.array_equal(bits(err), bits(s.kkt_error(mueq)))


def check_host_copy_dropped(lib_path, mueq=1e-10):
    """the eager state of backward_blocks (batch 1: the roll-out and the solution's copy to pinned memory run behind the
    sweep): after a refine the getters and fetch_results serve the refined solution, not that copy"""
    probs = singular_problems(8, 4, 4, 1)
    s = BatchedRiccatiSolver([k.dims for k in probs[0].stages], probs[0].nc0, batch=1, lib_path=lib_path)
    assert s.backward_blocks(probs[0], mueq) and s.forward()
    rec0 = s.fetch_results(0, gains=False)[0].copy()
    z0 = s.solution(0)
    # (an O(1) step: a solution served from the copy is O(1) away from the oracle's solve of the substituted problem)
    step_from_afar(s, probs, mueq, lib_path, np.random.default_rng(77), label="after backward_blocks")
    rec1 = s.fetch_results(0, gains=False)[0].copy()
    z1 = s.solution(0)
    assert not np.array_equal(rec0, rec1) and pc.maxdiff(z0[0], z1[0]) > 1e-3
    assert np.array_equal(bits(rec1), bits(ac.raw_solutions(s, lib_path)[0][:rec1.size]))
    assert np.array_equal(bits(np.concatenate(z1[0])), bits(rec1[:np.concatenate(z1[0]).size]))


def check_after_resolve(lib_path, mueq=1e-10):
    """case 11: upload_affine + backward_affine + forward + refine(1): within MARGIN of the full solve's distance"""
    probs = singular_problems(8, 4, 5, 2)
    rng = np.random.default_rng(61)
    new = [ac.substituted(p, rng) for p in probs]
    s = solved(probs, lib_path, mueq, BACKWARD="wave")
    full = solved(new, lib_path, mueq, BACKWARD="wave")
    ac.resolve(s, new)
    z0s = solutions(s)
    assert s.refine(1) == (1, 2)
    for b in range(2):
        ref = pc.oracle_serial(new[b], mueq)[2]
        d_re, d_full = ac.distance(s.solution(b), ref), ac.distance(full.solution(b), ref)
        ratio = d_re / max(d_full, EPS)
        print(f"refine after re-solve b={b}: distance {d_re:.3e} full solve {d_full:.3e} ratio {ratio:.3f}")
        WORST["distance"] = max(WORST["distance"], ratio)
        assert ratio <= MARGIN, (b, d_re, d_full)
    assert_step(s, new, z0s, mueq, lib_path, label="after re-solve")
    step_from_afar(s, new, mueq, lib_path, rng, label="after re-solve", BACKWARD="wave")


def untouched_by(s, lib_path, calls, code, match=""):
    """every call raises gar_hip error `code`; the solution, the knots and the factors keep their bits"""
    multi = s.devices is not None
    knots = s.download_packed()
    fac = None if multi else ac.raw_factors(s, lib_path)
    sol = None if multi else ac.raw_solutions(s, lib_path)
    for call in calls:
        with pytest.raises(RuntimeError, match=f"gar_hip error {code}.*{match}"):
            call()
    s.sync()
    assert np.array_equal(bits(knots), bits(s.download_packed()))
    if not multi:
        assert np.array_equal(bits(fac), bits(ac.raw_factors(s, lib_path)))
        assert np.array_equal(bits(sol), bits(ac.raw_solutions(s, lib_path)))


def both_forms(s):
    return (lambda: s.refine(1), lambda: s.refine_async(1), lambda: s.refine(2, 1e-9))


def check_refusals(lib_path, what, devices=(0, 0), mueq=1e-6):
    """case 12: the unserved kinds answer GAR_HIP_ERR_UNSUPPORTED, a missing backward or forward GAR_HIP_ERR_ARG"""
    nx, nu, N = 8, 4, 5
    if what == "nc":
        probs = kc.constrained(nx, nu, 2, N, 2, D=True)
        s = solved(probs, lib_path, mueq)
    elif what == "nth":
        rng = np.random.default_rng(37)
        probs = [synth.generate_lq_problem(rng, rng.standard_normal(nx), N, nx, nu, nth=2, mode="W", singular=False)
                 for _ in range(2)]
        s = solved(probs, lib_path, mueq)
    elif what == "legs":
        s = solved(kc.unconstrained(nx, nu, N, 2), lib_path, mueq, num_legs=2)
    elif what == "dense":
        s = solved(kc.unconstrained(nx, nu, N, 2), lib_path, mueq, dense=True)
    elif what == "multi":
        probs = kc.unconstrained(nx, nu, 11, 2)
        s = BatchedRiccatiSolver([k.dims for k in probs[0].stages], probs[0].nc0, batch=2, num_legs=4, lib_path=lib_path,
                                 devices=list(devices))
        s.upload(probs)
        assert s.backward(mueq) and s.forward()
    elif what == "no backward":
        s = kc.solver_for(kc.unconstrained(nx, nu, N, 2), lib_path)
        return untouched_by(s, lib_path, both_forms(s), -1, "no backward")
    elif what == "no forward":
        s = solved(kc.unconstrained(nx, nu, N, 2), lib_path, mueq)
        assert s.backward(mueq)
        untouched_by(s, lib_path, both_forms(s), -1, "no forward")
        assert s.forward() and s.refine(1) == (1, 2)
        return
    else:                                   # bad arguments
        s = solved(kc.unconstrained(nx, nu, N, 2), lib_path, mueq)
        return untouched_by(s, lib_path, (lambda: s.refine(-1), lambda: s.refine_async(-1), lambda: s.refine(1, np.nan),
                                          lambda: s.refine_async(1, np.nan)), -1)
    untouched_by(s, lib_path, both_forms(s), -3)


def check_invalidation(lib_path, mueq=1e-10):
    """case 12: new matrices end the refinement until the next backward"""
    nx, nu, N = 8, 4, 4
    probs, others = singular_problems(nx, nu, N, 2), kc.unconstrained(nx, nu, N, 2, seed=11)
    s = solved(probs, lib_path, mueq, BACKWARD="wave")
    steps_against_yardstick(s, probs, mueq, lib_path, steps=1, label="before new matrices")
    keep, ptr = ac.to_device(np.zeros(s.batch * s.deriv_doubles), lib_path)
    for upload, name in ((lambda: s.upload(others), "upload_stage|upload_packed"),
                         (lambda: s.upload_knot(0, 1, others[0].stages[1]), "upload_stage"),
                         (lambda: s.update_lq_subproblem_device(ptr, 1e-3, False), "update_lq_subproblem_device")):
        upload()
        s.sync()
        untouched_by(s, lib_path, both_forms(s), -1, f"({name})")
    s.upload(others)
    assert s.backward(mueq) and s.forward()
    steps_against_yardstick(s, others, mueq, lib_path, steps=1, label="after new matrices (a stale W fails here)")


def check_failed_problem(lib_path, mueq=1e-8):
    """case 13: problem 1 of three fails its backward; the refinement leaves it alone, solution included, refines the
    others and reports like the re-solve does"""
    nx, nu, N = 8, 4, 5
    probs = singular_problems(nx, nu, N, 3)
    bad = probs[1].stages[2]
    bad.R[...] = 0.0
    bad.S[...] = 0.0
    bad.B[...] = 0.0
    s = kc.solver_for(probs, lib_path, BACKWARD="wave")
    pc.assert_reported_failure(s.backward, mueq)
    st = s.status()
    assert [bool(v) for v in st] == [False, True, False]
    s.forward()
    fac, sol = ac.raw_factors(s, lib_path), ac.raw_solutions(s, lib_path)
    z0s = solutions(s, only=(0, 2))
    pc.assert_reported_failure(lambda _: s.refine(1), mueq)
    s.refine_async(0)                                              # (the asynchronous form does not wait: no report)
    s.sync()
    after = ac.raw_solutions(s, lib_path)
    assert np.array_equal(bits(sol[1]), bits(after[1]))
    assert not np.array_equal(bits(sol[0]), bits(after[0])) and not np.array_equal(bits(sol[2]), bits(after[2]))
    assert np.array_equal(bits(fac), bits(ac.raw_factors(s, lib_path)))
    assert np.array_equal(st, s.status()) and s.num_failed() == 1
    assert_step(s, probs, z0s, mueq, lib_path, label="failed batch")


def check_allocation(lib_path, rounds=20, mueq=1e-10):
    """case 14: the first call may allocate; twenty further ones do not, a backward in between included"""
    L = _lib.load(lib_path)
    probs = singular_problems(8, 4, 3, 3)
    s = solved(probs, lib_path, mueq)
    c0 = L.gar_hip_debug_alloc_count()
    s.refine(1)
    s.refine_async(1, 1e-12)
    s.sync()
    c1 = L.gar_hip_debug_alloc_count()
    assert 0 < c1 - c0 <= 9            # the KKT buffers (2), the re-solve's (3), the refinement's (4)
    for i in range(rounds):
        s.refine(2, 1e-13)
        s.refine_async(1)
        if i == rounds // 2:
            assert s.backward(mueq) and s.forward()
    s.sync()
    assert L.gar_hip_debug_alloc_count() == c1


def check_no_host_sync(lib_path, mueq=1e-10, pipeline=False):
    """case 15: backward_async -> forward_async -> refine_async -> refine_async -> sync"""
    probs = singular_problems(8, 4, 5, 5)
    s = kc.solver_for(probs, lib_path, BACKWARD="wave")
    once = kc.solver_for(probs, lib_path, BACKWARD="wave")
    if pipeline:
        for q in (s, once):
            q.set_pipeline(2)
            assert q.pipeline == 2
    once.backward_async(mueq)
    once.forward_async()
    once.refine_async(1)
    s.backward_async(mueq)
    s.forward_async()
    s.refine_async(1)
    s.refine_async(1)
    s.sync()
    once.sync()
    assert s.num_failed() == 0
    z0s = solutions(once)                          # the solution the second step started from
    label = "no host sync" + (" (pipelined)" if pipeline else "")
    assert_step(s, probs, z0s, mueq, lib_path, label=label)
    step_from_afar(s, probs, mueq, lib_path, np.random.default_rng(75), label=label, enqueued=True, BACKWARD="wave")


def check_default_batch(mueq=1e-10):
    """case 16 (GPU only): (36, 12), N = 16, batch 8 x #CUs -- the batch at which a new solver starts pipelined -- in
    mode "F" from synth_device.  Five problems spread over the batch against the yardstick; the batch-wide dualErr
    maximum after the step is not above the maximum before."""
    import torch
    from aligator_amd import synth_device
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nx, nu, N, batch = 36, 12, 16, 8 * cus
    dims = [(nx, nu, 0, nx, 0)] * N + [(nx, 0, 0, nx, 0)]
    spread = (0, 1, batch // 2 - 1, batch // 2, batch - 1)
    s = BatchedRiccatiSolver(dims, nx, batch=batch)
    assert s.pipeline == 2 and s.kernel_name == "wave<36,12>"
    synth_device.fill_problems(s, seed=11, mode="F")
    s.backward_async(mueq)
    s.forward_async()
    s.kkt_error_async(mueq)
    s.sync()
    assert s.num_failed() == 0
    before = kc.device_results(s, None)[0].copy()
    probs = {b: kc.host_problem(s, b) for b in spread}
    z0s = solutions(s, spread)
    s.refine_async(1)
    s.sync()
    after = kc.device_results(s, None)[0]
    print(f"refine default batch: device triple max before {before.max(axis=0)} after {after.max(axis=0)}")
    assert np.isfinite(after).all() and after[:, 2].max() <= before[:, 2].max()
    assert_step(s, probs, z0s, mueq, None, label="default batch")
    s.close()
