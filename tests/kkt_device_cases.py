"""Device-side KKT residuals and per-problem status (gar_hip_kkt_error, gar_hip_get_status; csrc/gar_kkt.hpp, DESIGN.md
5.3b): cases and checks shared by the emulator tests (tests/test_kkt_device.py) and the GPU tests
(tests/test_kkt_device_gpu.py).

The comparison: the device's triple and its per-stage norms against aligator_amd.lqr.lqrComputeKktError and a per-stage
host evaluation (stage_residuals below) on the problem and the solution downloaded from the SAME solver.  The tolerance
is derived: two fp64 evaluations of a row sum_k t_k with n addends differ by at most 2 n eps S_row, S_row = sum_k |t_k|;
S is the largest such row sum of a residual (the same formula with |block| @ |vector| and |rhs|) and
n = nx + nx2 + nu + nc + nth + nc0 + 4 counts more addends than any row has.

The check that matters: at the true solution every residual sits near 1e-13, where a kernel that returned zeros would
pass.  So every case is also run MISMATCHED -- after backward + forward another problem is uploaded and not swept --
where the residuals are O(1) and a dropped block, a transposed S, a wrong stage offset or ring slot is an O(1) error
against the same bound; and with separable changes (f, d, mueq, q, r, g0 of ONE problem of the batch), where only the
named slots of that problem may move and every other number must keep its bits."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from aligator_amd import _lib, synth
from aligator_amd.gar import BatchedRiccatiSolver
from aligator_amd.lqr import LqrProblem, lqrComputeKktError
import parity_cases as pc
import serial_fold_cases as sf

EPS = float(np.finfo(np.float64).eps)
DYN, CST, GX, GU = range(4)


# ---- host side: per-stage residuals and their row sums of absolute values -------------------------------------------
def stage_residuals(prob, sol, mueq, theta=None):
    """-> (norms (N+1, 4), S (N+1, 4), n (N+1,)): the four infinity norms dyn, cst, gx, gu per stage (utils.hxx:116-178;
    stage 0's dyn slot carries g0 + G0 x0, the terminal one is 0), the largest row sum of absolute values behind each,
    and the addend count of the bound."""
    xs, us, vs, lbdas = sol
    N = prob.horizon
    norms, S, n = np.zeros((N + 1, 4)), np.zeros((N + 1, 4)), np.zeros(N + 1)
    a = np.abs

    def inf(v):
        return float(np.max(np.abs(v))) if v.size else 0.0

    def top(v):
        return float(np.max(v)) if v.size else 0.0

    for t, k in enumerate(prob.stages):
        x, v = xs[t], vs[t]
        u = us[t] if k.nu > 0 else np.zeros(0)
        cst = k.C @ x + k.d - mueq * v
        s_cst = a(k.C) @ a(x) + a(k.d) + abs(mueq) * a(v)
        gx = k.q + k.Q @ x + k.C.T @ v
        s_gx = a(k.q) + a(k.Q) @ a(x) + a(k.C.T) @ a(v)
        gu = k.r + k.S.T @ x + k.D.T @ v
        s_gu = a(k.r) + a(k.S.T) @ a(x) + a(k.D.T) @ a(v)
        if k.nu > 0:
            cst, s_cst = cst + k.D @ u, s_cst + a(k.D) @ a(u)
            gx, s_gx = gx + k.S @ u, s_gx + a(k.S) @ a(u)
            gu, s_gu = gu + k.R @ u, s_gu + a(k.R) @ a(u)
        dyn_n, s_dyn = 0.0, 0.0
        if t == 0:
            gx, s_gx = gx + prob.G0.T @ lbdas[0], s_gx + a(prob.G0.T) @ a(lbdas[0])
            dyn_n = inf(prob.g0 + prob.G0 @ x)
            s_dyn = top(a(prob.g0) + a(prob.G0) @ a(x))
        else:
            gx, s_gx = gx - lbdas[t], s_gx + a(lbdas[t])
        if t < N:
            dyn = k.A @ x + k.B @ u + k.f - xs[t + 1]
            dyn_n = max(dyn_n, inf(dyn)) if not np.isnan(inf(dyn)) else float("nan")
            s_dyn = max(s_dyn, top(a(k.A) @ a(x) + a(k.B) @ a(u) + a(k.f) + a(xs[t + 1])))
            gx, s_gx = gx + k.A.T @ lbdas[t + 1], s_gx + a(k.A.T) @ a(lbdas[t + 1])
            gu, s_gu = gu + k.B.T @ lbdas[t + 1], s_gu + a(k.B.T) @ a(lbdas[t + 1])
        nth = 0
        if theta is not None:
            nth = k.nth
            gx, s_gx = gx + k.Gx @ theta, s_gx + a(k.Gx) @ a(theta)
            gu, s_gu = gu + k.Gu @ theta, s_gu + a(k.Gu) @ a(theta)
        norms[t] = dyn_n, inf(cst), inf(gx), inf(gu)
        S[t] = s_dyn, top(s_cst), top(s_gx), top(s_gu)
        n[t] = k.nx + k.nx2 + k.nu + k.nc + nth + prob.nc0 + 4
    return norms, S, n


def host_problem(s, b):
    """problem b as the solver holds it (download_packed), in the caller's dimensions"""
    return s.unpack(s.download_packed(b, 1))


def theta_of(theta, s, b):
    if theta is None:
        return None
    nth = int(s.dims[0, 4])
    return np.asarray(theta, dtype=np.float64).reshape(s.batch, nth)[b]


def assert_matches_host(s, mueq, theta=None, problems=None, only=None):
    """The device's triples and stage norms of every problem (or of `only`) against the host's, within 2 n eps S.  Prints
    the largest difference over its bound.  Returns (triples, stage norms) of the device."""
    err, st = s.kkt_error(mueq, theta, stages=True)
    assert err.shape == (s.batch, 3) and st.shape == (s.batch, s.horizon + 1, 4)
    worst = 0.0
    for b in (range(s.batch) if only is None else only):
        prob = problems[b] if problems is not None else host_problem(s, b)
        sol = s.solution(b)
        th = theta_of(theta, s, b)
        norms, S, n = stage_residuals(prob, sol, mueq, th)
        bound = 2.0 * n[:, None] * EPS * S
        assert np.isfinite(norms).all() and np.isfinite(st[b]).all(), b
        diff = np.abs(st[b] - norms)
        assert (diff <= bound).all(), (b, np.argwhere(diff > bound).tolist(), diff.max(), bound.max())
        worst = max(worst, float((diff / np.maximum(bound, 1e-300)).max()))
        ref = lqrComputeKktError(prob, *sol, mueq=mueq, theta=th)
        tb = bound.max(axis=0)
        for got, want, bd in zip(err[b], ref, (tb[DYN], tb[CST], max(tb[GX], tb[GU]))):
            assert abs(got - want) <= bd, (b, got, want, bd)
        # the triple is the fold of the stage norms, exactly
        assert err[b, 0] == st[b, :, DYN].max() and err[b, 1] == st[b, :, CST].max()
        assert err[b, 2] == st[b, :, GX:].max()
        assert s.horizon == 0 or st[b, s.horizon, DYN] == 0.0      # (one knot: the slot is the initial condition's)
    print(f"kkt device-host: largest |diff| / bound = {worst:.3f}")
    return err, st


def moved(base, now, b, slots):
    """Between two device results: exactly the (stage, slot) pairs `slots` of problem b differ, every other number of
    the batch -- the triples of the other problems included -- keeps its bits."""
    (e0, s0), (e1, s1) = base, now
    changed = {(int(t), int(k)) for t, k in np.argwhere(s0[b] != s1[b])}
    assert changed == set(slots), (sorted(changed), sorted(slots))
    keep = np.ones(s0.shape[0], dtype=bool)
    keep[b] = False
    assert np.array_equal(s0[keep], s1[keep]) and np.array_equal(e0[keep], e1[keep])


# ---- the two forms of every case ------------------------------------------------------------------------------------
def check_true_and_mismatched(s, probs, mueq, other, b=0, theta=None, stages=None):
    """probs: the batch already uploaded into s; other: a problem of the same dimensions that the solution of problem b
    does not solve.  Sweeps once, then never again."""
    N = s.horizon
    assert s.backward(mueq) and s.forward(theta) and s.num_failed() == 0
    assert not s.status().any()
    base = assert_matches_host(s, mueq, theta)
    # (1) another problem under the same solution: O(1) residuals, the same bound
    s.upload([other], b)
    now = assert_matches_host(s, mueq, theta)
    assert now[0][b].max() > 1e-3, now[0][b]
    keep = np.arange(s.batch) != b
    assert np.array_equal(base[0][keep], now[0][keep]) and np.array_equal(base[1][keep], now[1][keep])
    # (2) separable changes of problem b, each from the swept problem
    ts = stages if stages is not None else sorted({min(1, N), max(N - 1, 0)})
    p0 = probs[b]

    def variant(edit):
        q = p0.copy()
        edit(q)
        s.upload([q], b)
        return assert_matches_host(s, mueq, theta, only=[b])

    def bump(name, t):
        def edit(q):
            getattr(q.stages[t], name)[...] += 1.0 + 0.25 * np.arange(getattr(q.stages[t], name).size)
        return edit
    tf = [t for t in ts if t < N]
    if tf:
        def edit_f(q):
            for t in tf:
                bump("f", t)(q)
        moved(base, variant(edit_f), b, [(t, DYN) for t in tf])
    tq = ts[0]
    moved(base, variant(bump("q", tq)), b, [(tq, GX)])
    tr = [t for t in ts if p0.stages[t].nu > 0]
    if tr:
        moved(base, variant(bump("r", tr[0])), b, [(tr[0], GU)])
    tc = [t for t in range(N + 1) if p0.stages[t].nc > 0]
    if tc:
        moved(base, variant(bump("d", tc[-1])), b, [(tc[-1], CST)])
    if p0.nc0 > 0:
        def edit_g0(q):
            q.g0[...] += 1.0
        moved(base, variant(edit_g0), b, [(0, DYN)])
    # back to the swept problem: the bits of the first evaluation
    s.upload([p0], b)
    again = s.kkt_error(mueq, theta, stages=True)
    assert np.array_equal(again[0], base[0]) and np.array_equal(again[1], base[1])
    if tc:  # only the mueq passed: only cst moves, on every problem, at the constrained stages with a multiplier
        other_mu = s.kkt_error(2.0 * mueq + 0.5, theta, stages=True)
        diff = np.argwhere(other_mu[1] != base[1])
        assert len(diff) > 0 and set(int(k) for k in diff[:, 2]) == {CST}
        assert set(int(t) for t in diff[:, 1]) <= set(tc)
        for bb in range(s.batch):
            prob, sol = host_problem(s, bb), s.solution(bb)
            norms, S, n = stage_residuals(prob, sol, 2.0 * mueq + 0.5, theta_of(theta, s, bb))
            assert (np.abs(other_mu[1][bb] - norms) <= 2.0 * n[:, None] * EPS * S).all()
    return base


@contextlib.contextmanager
def options(**kv):
    with sf.options(**kv):
        yield


def solver_for(probs, lib_path, num_legs=1, dense=False, **opts):
    with options(**opts):
        s = BatchedRiccatiSolver([k.dims for k in probs[0].stages], probs[0].nc0, batch=len(probs), num_legs=num_legs,
                                 lib_path=lib_path, dense=dense)
    s.upload(probs)
    return s


def unconstrained(nx, nu, N, batch, seed=0):
    rng = np.random.default_rng([seed, nx, nu, N])
    return [synth.generate_lq_problem(rng, rng.standard_normal(nx), N, nx, nu, mode="W", singular=False)
            for _ in range(batch)]


def constrained(nx, nu, nc, N, batch, D, seed=0):
    rng = np.random.default_rng([seed, nx, nu, nc, N])
    out = []
    for _ in range(batch):
        p = synth.generate_lq_problem(rng, rng.standard_normal(nx), N, nx, nu, nc=nc, mode="W", singular=False)
        for k in p.stages:
            k.C[...] = rng.uniform(-1, 1, k.C.shape)
            if D:
                k.D[...] = rng.uniform(-1, 1, k.D.shape)
        out.append(p)
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------
def check_serial(lib_path, nx, nu, N, batch, family, kernel, qr_packed, mueq=1e-8):
    """(8, 4) on wave / wg4 and (36, 12): packed Q / R (the one-wave family) and full records"""
    probs = unconstrained(nx, nu, N, batch + 1)
    s = solver_for(probs[:batch], lib_path, BACKWARD=family)
    assert s.kernel_name == kernel, s.kernel_name
    assert bool(s.record_format & 1) == qr_packed, s.record_format
    check_true_and_mismatched(s, probs[:batch], mueq, probs[batch], b=batch - 1)


def check_constrained_serial(lib_path, nx, nu, nc, N, D, kernel, mueq=1e-4, **opts):
    """(36, 12, 32) with D = 0 / a random D (the coupled stage), (8, 4, 4) on the any-dimension kernels"""
    probs = constrained(nx, nu, nc, N, 3, D)
    s = solver_for(probs[:2], lib_path, **opts)
    assert s.kernel_name == kernel, s.kernel_name
    check_true_and_mismatched(s, probs[:2], mueq, probs[2], b=1)
    if D and kernel.startswith("wave<"):
        assert sum(s.constrained_bk_stages()) > 0   # the coupled stage (or the LDS Bunch-Kaufman) ran


def check_mixed_nc(lib_path, fold, mueq=1e-6):
    """case B of serial_fold_cases (constraints on knots 1, 3, 5 only), with and without SERIAL_FOLD=1"""
    probs = sf.make_batch("B")
    other = sf.make_problem("B", 999)
    s = solver_for(probs, lib_path, SERIAL_FOLD="1" if fold else None, BACKWARD="wave")
    assert s.kernel_name == ("wave<8,4>+fold" if fold else "generic"), s.kernel_name
    assert s.record_format == 0
    check_true_and_mismatched(s, probs, mueq, other, b=1, stages=[1, 3])


def check_padded(lib_path, nx, nu, N, kernel, mueq=1e-8):
    """(4, 2) -> (8, 4), (12, 6) -> (12, 8), (56, 22) -> (56, 24): the host side works in the caller's dimensions -- the
    dummy states and controls must add exactly nothing to any norm"""
    probs = unconstrained(nx, nu, N, 3)
    s = solver_for(probs[:2], lib_path, BACKWARD="wave")      # (the family would follow batch vs. #CUs otherwise)
    assert s.padded and s.kernel_name == kernel, (s.padded, s.kernel_name)
    check_true_and_mismatched(s, probs[:2], mueq, probs[2], b=0)


def check_legs(lib_path, kind, mueq=1e-6):
    """leg mode: wave legs (8, 4), N = 11, 3 uneven legs; the same with state-only constraints (leg fold); the
    constrained segment legs (8, 4, 4), N = 9"""
    if kind == "plain":
        probs, kernel = unconstrained(8, 4, 11, 3), "wave_leg<8,4>"
    elif kind == "fold":
        probs, kernel = constrained(8, 4, 3, 11, 3, D=False), "wave_leg<8,4>+fold"
    else:
        probs, kernel = constrained(8, 4, 4, 9, 3, D=True), "wave_leg<8,4>+fold|wave_seg<8,4,4>"
    s = solver_for(probs[:2], lib_path, num_legs=3)
    assert s.kernel_name == kernel, s.kernel_name
    check_true_and_mismatched(s, probs[:2], mueq, probs[2], b=1, stages=[3, 4])   # either side of a leg boundary
    with pytest.raises(RuntimeError, match="gar_hip error -1"):     # theta has no say in leg mode: GAR_HIP_ERR_ARG
        s.kkt_error(mueq, theta=np.zeros(8 * 2))


def check_dense(lib_path, mueq=1e-4):
    probs = constrained(6, 3, 2, 4, 3, D=True)
    s = solver_for(probs[:2], lib_path, dense=True)
    assert s.kernel_name == "dense", s.kernel_name
    check_true_and_mismatched(s, probs[:2], mueq, probs[2], b=0)


def check_parameterised(lib_path, mueq=1e-8):
    """(10, 4), nth = 2, N = 6: with a theta (the Gx, Gu columns enter) and with NULL; the three refusals"""
    nx, nu, nth, N = 10, 4, 2, 6
    rng = np.random.default_rng(31)
    probs = [synth.generate_lq_problem(rng, rng.standard_normal(nx), N, nx, nu, nth=nth, mode="W", singular=False)
             for _ in range(3)]
    theta = rng.standard_normal((2, nth))
    for th in (theta, None):
        s = solver_for(probs[:2], lib_path)
        check_true_and_mismatched(s, probs[:2], mueq, probs[2], b=1, theta=th)
    # a theta moves gx and gu of every stage against the NULL evaluation, nothing else
    with_th, without = s.kkt_error(mueq, theta, stages=True), s.kkt_error(mueq, None, stages=True)
    diff = np.argwhere(with_th[1] != without[1])
    assert set(int(k) for k in diff[:, 2]) == {GX, GU} and len(diff) >= 2 * N
    plain = solver_for(unconstrained(nx, nu, N, 2), lib_path)
    assert plain.backward(mueq) and plain.forward()
    with pytest.raises(RuntimeError, match="gar_hip error -1"):     # nth = 0: GAR_HIP_ERR_ARG
        plain.kkt_error(mueq, theta=np.zeros(4))
    with pytest.raises(RuntimeError, match="gar_hip error -1"):
        plain.kkt_error_async(mueq, theta_device_ptr=theta.ctypes.data)
    # stages that differ in nth: no Gx theta, Gu theta of EVERY stage exists, so a theta is refused (checked before any launch)
    mixed = BatchedRiccatiSolver([(nx, nu, 0, nx, nth)] * N + [(nx, 0, 0, nx, 0)], nx, batch=2, lib_path=lib_path)
    with pytest.raises(RuntimeError, match="gar_hip error -1"):
        mixed.kkt_error(mueq, theta=np.zeros(2 * nth))


def check_terminal_nx2_zero(lib_path, mueq=1e-8):
    """the terminal knot as ProxDDP builds it: nx2 = 0, nu = 0 (kept as nx2 = nx in the records)"""
    nx, nu, N = 8, 4, 4
    rng = np.random.default_rng(17)
    probs = []
    for _ in range(3):
        knots = [synth.generate_knot(rng, nx, nu, mode="W") for _ in range(N)]
        knots.append(synth.generate_knot(rng, nx, 0, nx2=0, mode="W"))
        p = LqrProblem(knots, nx)
        p.G0[...] = -np.eye(nx)
        p.g0[...] = rng.standard_normal(nx)
        probs.append(p)
    s = solver_for(probs[:2], lib_path)
    assert tuple(s.dims[N]) == (nx, 0, 0, 0, 0) and int(s.packed_dims[N, 3]) == nx
    check_true_and_mismatched(s, probs[:2], mueq, probs[2], b=0)


def check_one_knot(lib_path, mueq=1e-8):
    """N = 0: one knot, no dynamics -- the dyn slot is the initial condition's"""
    probs = unconstrained(6, 3, 0, 3)
    s = solver_for(probs[:2], lib_path)
    assert s.horizon == 0
    check_true_and_mismatched(s, probs[:2], mueq, probs[2], b=1)


def check_ring(lib_path, family="wave", mueq=1e-8):
    """(8, 4), N = 5: two cycleAppends (a ring: no record moves), only the new knots uploaded, then the sweep; the host
    side is the caller's own rotated problem.  Mismatched: f of LOGICAL stage 1 moves stage slot 1 of the output."""
    nx, nu, N = 8, 4, 5
    probs = unconstrained(nx, nu, N, 2)
    rng = np.random.default_rng(5)
    s = solver_for(probs, lib_path, BACKWARD=family)
    assert s.backward(mueq) and s.forward()
    for _ in range(2):
        s.cycle_append(probs[0].stages[0].dims)
        for b, p in enumerate(probs):
            new = synth.generate_knot(rng, nx, nu, mode="W")
            p.stages[:N] = p.stages[1:N] + [new]
            s.upload_knot(b, N - 1, new)
    assert int(s.stage_offsets[0, 0]) != int(s.stage_offsets[:, 0].min())      # the ring has turned
    assert s.backward(mueq) and s.forward() and s.num_failed() == 0
    for b, p in enumerate(probs):       # what the solver holds is the caller's rotated problem (Q, R: their lower triangles)
        got = host_problem(s, b)
        for k, g in zip(p.stages, got.stages):
            for name in ("S", "q", "r", "A", "B", "f"):
                assert np.array_equal(getattr(k, name), getattr(g, name))
            assert np.array_equal(np.tril(k.Q), np.tril(g.Q)) and np.array_equal(np.tril(k.R), np.tril(g.R))
    base = assert_matches_host(s, mueq)
    k1 = probs[1].stages[1].copy()
    k1.f[...] += 1.0 + np.arange(nx)
    s.upload_knot(1, 1, k1)
    now = assert_matches_host(s, mueq)
    moved(base, now, 1, [(1, DYN)])
    assert now[1][1, 1, DYN] > 0.5


def check_grid(lib_path, mueq=1e-8):
    """(8, 4), N = 2, batch 70: more problems than lanes in a wave, more than one block of any block size up to 256
    (in units of problems or of (problem, stage) pairs); problems 0, 63, 64 and 69 perturbed one at a time"""
    nx, nu, N, batch = 8, 4, 2, 70
    few = unconstrained(nx, nu, N, 7)
    probs = [few[b % 7].copy() for b in range(batch)]
    for b, p in enumerate(probs):
        p.g0[...] += 0.01 * b
    s = solver_for(probs, lib_path)
    assert s.backward(mueq) and s.forward() and s.num_failed() == 0
    base = assert_matches_host(s, mueq, only=[0, 1, 63, 64, 69])
    assert (base[0] < 1e-9).all()
    for b in (0, 63, 64, 69):
        q = probs[b].copy()
        q.stages[1].f[...] += 1.0 + b
        s.upload([q], b)
        now = assert_matches_host(s, mueq, only=[b])
        moved(base, now, b, [(1, DYN)])
        s.upload([probs[b]], b)


def read_device(ptr, n, lib_path):
    """n doubles at the device address ptr (the emulator's device memory is host memory)"""
    if lib_path is not None:
        return np.ctypeslib.as_array((C.c_double * n).from_address(ptr)).copy()
    import torch  # noqa: F401  (the HIP runtime torch already loaded)
    out = np.zeros(n)
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(8 * n), 2) == 0
    return out


def device_results(s, lib_path):
    pe, ps = s.device_kkt_errors()
    assert pe and ps
    return (read_device(pe, s.batch * 3, lib_path).reshape(s.batch, 3),
            read_device(ps, s.batch * (s.horizon + 1) * 4, lib_path).reshape(s.batch, s.horizon + 1, 4))


def check_pipelined(lib_path, mueq=1e-8):
    """set_pipeline(2), (8, 4), N = 5, batch 5 (uneven halves): backward_async + forward_async + kkt_error_async with no
    host synchronisation in between, then sync -- bitwise the plain schedule's result"""
    probs = unconstrained(8, 4, 5, 5)
    s = solver_for(probs, lib_path, BACKWARD="wave")
    assert s.device_kkt_errors() == (None, None)
    s.set_pipeline(0)
    s.backward_async(mueq)
    s.forward_async()
    s.kkt_error_async(mueq)
    s.sync()
    plain = device_results(s, lib_path)
    assert_matches_host(s, mueq)
    s.set_pipeline(2)
    assert s.pipeline == 2
    for _ in range(2):
        s.backward_async(mueq)
        s.forward_async()
        s.kkt_error_async(mueq)
    s.sync()
    piped = device_results(s, lib_path)
    assert np.array_equal(plain[0], piped[0]) and np.array_equal(plain[1], piped[1])
    assert s.num_failed() == 0 and not s.status().any()


def check_failures(lib_path):
    """the batch of four at mueq = 0 of parity_cases.check_mueq_batch_of_four: the reference fails on problems 1 and 3"""
    nx, nu, nc, N = 8, 4, 4, 5
    good = [synth.mueq_problem("mixed", nx, nu, nc, N, seed=sd) for sd in (0, 1)]
    bad = [p.copy() for p in good]
    for p in bad:
        for k in p.stages:
            k.D[...] = 0.0
    probs = [good[0], bad[0], good[1], bad[1]]
    assert [pc.reference_solvable(p, 0.0) for p in probs] == [True, False, True, False]
    s = solver_for(probs, lib_path, num_legs=3)
    assert s.kernel_name == f"wave_leg<{nx},{nu}>+fold"
    pc.assert_reported_failure(s.backward, 0.0)
    st = s.status()
    assert st.dtype == np.int32 and st.shape == (4,)
    assert [bool(v) for v in st] == [False, True, False, True], st
    assert s.num_failed() == int((st != 0).sum()) == 2
    s.forward()
    err, stage = s.kkt_error(0.0, stages=True)
    assert_matches_host(s, 0.0, only=[0, 2])
    for b in (1, 3):
        flat = np.concatenate([np.ravel(v) for part in s.solution(b) for v in part])
        if not np.isfinite(flat).all():
            assert not np.isfinite(err[b]).all(), (b, err[b])


def check_allocation(lib_path, rounds=20, mueq=1e-8):
    """create allocates what it did before these calls existed; the first kkt_error may allocate; 20 further rounds of
    backward / forward / kkt_error do not; after a rebuilding cycleAppend the calls work again"""
    L = _lib.load(lib_path)
    nx, nu, N = 8, 4, 3
    probs = unconstrained(nx, nu, N, 3)
    c0 = L.gar_hip_debug_alloc_count()
    never = solver_for(probs[:2], lib_path)         # an identical solver on which the new calls are never made
    c1 = L.gar_hip_debug_alloc_count()
    s = solver_for(probs[:2], lib_path)
    c2 = L.gar_hip_debug_alloc_count()
    assert c2 - c1 == c1 - c0 > 0
    assert s.device_kkt_errors() == (None, None)
    assert s.backward(mueq) and s.forward()
    assert never.backward(mueq) and never.forward()
    c3 = L.gar_hip_debug_alloc_count()
    assert c3 == c2                                   # (neither sweep allocated)
    first = s.kkt_error(mueq)
    c4 = L.gar_hip_debug_alloc_count()
    assert 0 <= c4 - c3 <= 2
    ptrs = s.device_kkt_errors()
    assert all(ptrs)
    for _ in range(rounds):
        assert s.backward(mueq) and s.forward()
        assert np.array_equal(s.kkt_error(mueq), first)
        s.kkt_error_async(mueq)
        s.status()
    s.sync()
    assert L.gar_hip_debug_alloc_count() == c4 and s.device_kkt_errors() == ptrs
    # a cycleAppend that changes the dimensions rebuilds the layout: the buffers go with it, the next call makes them again
    s.cycle_append((nx, nu, 2, nx, 0))
    assert s.device_kkt_errors() == (None, None)
    rng = np.random.default_rng(3)
    new = []
    for p in probs[:2]:
        q = p.copy()
        k = synth.generate_knot(rng, nx, nu, 2, mode="W")
        q.stages[:N] = q.stages[1:N] + [k]
        new.append(q)
    s.upload(new)
    assert s.backward(1e-4) and s.forward()
    assert_matches_host(s, 1e-4)
    assert all(s.device_kkt_errors())


def check_multi_device(lib_path, devices=(0, 0), mueq=1e-8):
    """a multi-device handle (two virtual devices on the emulator, the same device twice on the GPU): both calls answer
    GAR_HIP_ERR_UNSUPPORTED, the device pointers are NULL; the status words are served"""
    probs = unconstrained(8, 4, 11, 2)
    s = BatchedRiccatiSolver([k.dims for k in probs[0].stages], probs[0].nc0, batch=2, num_legs=4, lib_path=lib_path,
                             devices=list(devices))
    s.upload(probs)
    assert s.backward(mueq) and s.forward()
    with pytest.raises(RuntimeError, match="gar_hip error -3"):
        s.kkt_error(mueq)
    with pytest.raises(RuntimeError, match="gar_hip error -3"):
        s.kkt_error_async(mueq)
    assert s.device_kkt_errors() == (None, None)
    assert not s.status().any()
