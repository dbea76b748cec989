"""Gradients of a resident batch (gar_hip_adjoint, csrc/gar_adjoint.hpp, aligator_amd/layer.py): cases
and checks shared by the emulator tests (tests/test_adjoint.py) and the GPU tests (tests/test_adjoint_gpu.py).

Three yardsticks, none of them the code under test.
* The adjoint d.  d is the LQ solution for the same matrices and q, r, f, g0 := the cotangent (random, O(1), seeded): the
  ORACLE solves that substituted problem.  e_ref = the distance of the library's own FULL solve of it, on a fresh solver,
  to the oracle's, floored at one eps of the solution's scale; the adjoint may exceed e_ref by affine_cases.MARGIN = 10
  (an explicit inverse of R-hat and the stored, rounded K and Aff).
* The gradient blocks, indexing.  Every entry of the gradient record is a b + c d (halved exactly for Q and R) of entries
  of the DOWNLOADED solution and adjoint of the same call: three roundings, or two with an FMA, so
  |entry - numpy's| <= 4 eps (|a b| + |c d|) (halved for Q, R); the affine slots equal d and the pads are zero, exactly.
* The gradient blocks, end to end.  torch.autograd in fp64 on the CPU through torch.linalg.solve of the dense KKT matrix
  assembled from leaf tensors (Q, R entering as 1/2 (M + M^T)), loss = sum(w z), on generator "W" problems, after the
  premise that oracle/dense_kkt.py and the torch assembly agree on the solution to 1e-10.  e_ref = the error against
  autograd of the numpy formula on the ORACLE's solution and adjoint; the bar is max(1e-11 of the gradient's largest
  entry, 10 e_ref).
Every check prints its ratio; report() prints the largest seen (each module's docstring quotes them)."""
import numpy as np
import pytest

from aligator_amd import _lib, synth
from aligator_amd.gar import BatchedRiccatiSolver
from aligator_amd.lqr import LqrProblem
import affine_cases as ac
import init_stage_cases as isc
import kkt_device_cases as kc
import parity_cases as pc
import refine_cases as rc
from oracle import dense_kkt

EPS = kc.EPS
MARGIN = ac.MARGIN
WORST = {"adjoint": 0.0, "formula": 0.0, "autograd": 0.0}
bits = rc.bits


def report():
    print(f"adjoint over the full solve of the substituted problem: largest ratio {WORST['adjoint']:.3f} (margin {MARGIN:g}); "
          f"gradient entries over 4 eps (|ab| + |cd|): {WORST['formula']:.3f}; gradient against autograd over its bar: "
          f"{WORST['autograd']:.3f}")


# ---- vectors of the affine layout ----------------------------------------------------------------------------------------
def slot_N(s):
    """entries of the terminal knot's f / lbd slot in an affine-layout vector (a knot given with nx2 = 0 has none)"""
    return int(s.dims[s.horizon, 3])


def sol_to_vec(s, sol):
    """(xs, us, vs, lbdas) -> x_t | u_t | lbd_{t+1} per stage, then lbd0 (the terminal slot, where there is one: zeros)"""
    xs, us, _, lbdas = sol
    N, parts = s.horizon, []
    for t in range(N + 1):
        parts.append(xs[t])
        if int(s.dims[t, 1]) > 0:
            parts.append(us[t])
        parts.append(lbdas[t + 1] if t < N else np.zeros(slot_N(s)))
    parts.append(lbdas[0])
    out = np.concatenate([np.ravel(p) for p in parts])
    assert out.size == s.affine_doubles
    return out


def vec_to_sol(s, vec):
    xs, us, lbdas, p = [], [], [None], 0
    N = s.horizon
    for t in range(N + 1):
        nx, nu = int(s.dims[t, 0]), int(s.dims[t, 1])
        n2 = int(s.dims[t, 3]) if t < N else slot_N(s)
        xs.append(vec[p:p + nx]), us.append(vec[p + nx:p + nx + nu])
        if t < N:
            lbdas.append(vec[p + nx + nu:p + nx + nu + n2])
        p += nx + nu + n2
    lbdas[0] = vec[p:p + s.nc0]
    assert p + s.nc0 == vec.size
    return xs, us, lbdas


def with_affine(s, prob, vec):
    """`prob` with q, r, f, g0 := the entries of an affine-layout vector"""
    cp, p = prob.copy(), 0
    for k in cp.stages:
        for name in ("q", "r", "f"):
            blk = getattr(k, name)
            blk[...] = vec[p:p + blk.size]
            p += blk.size
    cp.g0[...] = vec[p:p + cp.g0.size]
    assert p + cp.g0.size == vec.size
    return cp


def cotangents(s, rng):
    return rng.standard_normal((s.batch, s.affine_doubles))


def vec_distance(got, ref):
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


# ---- the formulas in numpy -------------------------------------------------------------------------------------------------
def formula(s, prob, z, d):
    """-> (gradient record, bound record) of one problem from the affine-layout vectors z (solution) and d (adjoint): the
    caller's packed layout (BatchedRiccatiSolver.pack); bound = 4 eps (|a b| + |c d|), halved with the entry for Q, R, and
    zero on the affine slots and the pads"""
    xs, us, ls = vec_to_sol(s, z)
    dxs, dus, dls = vec_to_sol(s, d)
    G, B = prob.copy(), prob.copy()
    N = s.horizon

    def two(a, b, c, dd, half=False):
        f = 0.5 if half else 1.0
        return f * (np.outer(a, b) + np.outer(c, dd)), f * 4.0 * EPS * (np.abs(np.outer(a, b)) + np.abs(np.outer(c, dd)))

    for t, (g, bd) in enumerate(zip(G.stages, B.stages)):
        x, u, dx, du = xs[t], us[t], dxs[t], dus[t]
        g.Q[...], bd.Q[...] = two(dx, x, x, dx, half=True)
        g.S[...], bd.S[...] = two(dx, u, x, du)
        g.R[...], bd.R[...] = two(du, u, u, du, half=True)
        g.q[...], g.r[...] = dx, du
        bd.q[...], bd.r[...] = 0.0, 0.0
        if t < N:
            l, dl = ls[t + 1], dls[t + 1]
            g.A[...], bd.A[...] = two(dl, x, l, dx)
            g.B[...], bd.B[...] = two(dl, u, l, du)
            g.f[...] = dl
        else:
            g.A[...], g.B[...], g.f[...] = 0.0, 0.0, 0.0
            bd.A[...], bd.B[...] = 0.0, 0.0
        bd.f[...] = 0.0
    G.G0[...], B.G0[...] = two(dls[0], xs[0], ls[0], dxs[0])
    G.g0[...], B.g0[...] = dls[0], 0.0
    return s.pack(G), s.pack(B)


# ---- the yardsticks --------------------------------------------------------------------------------------------------------
def assert_adjoint(s, probs, cot, adj, mueq, lib_path, label="", only=None, **opts):
    """adj against the oracle's solve of the substituted problems, within MARGIN of the library's own full solve"""
    sub = [with_affine(s, p, c) for p, c in zip(probs, cot)]
    full = rc.solved(sub, lib_path, mueq, **opts)
    assert full.kernel_name == s.kernel_name
    for b in (range(s.batch) if only is None else only):
        ref = sol_to_vec(s, pc.oracle_serial(sub[b], mueq)[2])
        d_adj, d_full = vec_distance(adj[b], ref), vec_distance(sol_to_vec(s, full.solution(b)), ref)
        ratio = d_adj / max(d_full, EPS)
        print(f"adjoint {label} b={b}: distance {d_adj:.3e} full solve {d_full:.3e} ratio {ratio:.3f}")
        WORST["adjoint"] = max(WORST["adjoint"], ratio)
        assert np.isfinite(adj[b]).all() and ratio <= MARGIN, (label, b, ratio)
    full.close()
    report()


def assert_formula(s, probs, adj, grad, label="", only=None):
    """every entry of the gradient records against numpy's on the downloaded solution and adjoint"""
    for b in (range(s.batch) if only is None else only):
        z = sol_to_vec(s, s.solution(b))
        want, bound = formula(s, probs[b], z, adj[b])
        err = np.abs(grad[b] - want)
        ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        print(f"adjoint {label} b={b}: gradient entries over their bound {ratio:.3f}, largest entry {np.abs(want).max():.3e}")
        WORST["formula"] = max(WORST["formula"], ratio)
        assert np.isfinite(grad[b]).all() and (err <= bound).all(), (label, b, ratio, int(np.argmax(err - bound)))
        assert np.abs(want).max() > 0
        G = s.unpack_gradient(grad[b])                                   # Q, R: both triangles, bitwise symmetric
        for k in G.stages:
            assert np.array_equal(bits(k.Q), bits(k.Q.T)) and np.array_equal(bits(k.R), bits(k.R.T))
    report()


def autograd_record(s, prob, w, mueq=0.0):
    """-> (gradient record, solution vector) of loss = sum(w z) by torch.autograd through torch.linalg.solve of the dense
    KKT matrix assembled from leaf tensors; w and the solution in the affine layout"""
    import torch
    N, nc0 = s.horizon, prob.nc0
    leaf = lambda a: torch.tensor(np.array(a, dtype=np.float64), dtype=torch.float64, requires_grad=True)
    L = [{n: leaf(getattr(k, n)) for n in ("Q", "S", "R", "q", "r", "A", "B", "f")} for k in prob.stages]
    G0, g0 = leaf(prob.G0), leaf(prob.g0)
    n = nc0 + sum(k.nx + k.nu + (k.nx2 if t < N else 0) for t, k in enumerate(prob.stages))
    mat, rhs = torch.zeros((n, n), dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    nx0 = prob.stages[0].nx
    mat[:nc0, nc0:nc0 + nx0] = G0
    mat[nc0:nc0 + nx0, :nc0] = G0.T
    rhs[:nc0] = g0
    i = nc0
    for t, (k, m) in enumerate(zip(prob.stages, L)):
        nx, nu, n2 = k.nx, k.nu, k.nx2
        mat[i:i + nx, i:i + nx] = 0.5 * (m["Q"] + m["Q"].T)
        mat[i:i + nx, i + nx:i + nx + nu] = m["S"]
        mat[i + nx:i + nx + nu, i:i + nx] = m["S"].T
        mat[i + nx:i + nx + nu, i + nx:i + nx + nu] = 0.5 * (m["R"] + m["R"].T)
        rhs[i:i + nx], rhs[i + nx:i + nx + nu] = m["q"], m["r"]
        if t < N:
            r0 = i + nx + nu
            mat[r0:r0 + n2, i:i + nx], mat[i:i + nx, r0:r0 + n2] = m["A"], m["A"].T
            mat[r0:r0 + n2, i + nx:i + nx + nu], mat[i + nx:i + nx + nu, r0:r0 + n2] = m["B"], m["B"].T
            mat[r0:r0 + n2, r0 + n2:r0 + 2 * n2] = -torch.eye(n2, dtype=torch.float64)
            mat[r0 + n2:r0 + 2 * n2, r0:r0 + n2] = -torch.eye(n2, dtype=torch.float64)
            rhs[r0:r0 + n2] = m["f"]
            i += nx + nu + n2
    z = -torch.linalg.solve(mat, rhs)
    body = w.size - nc0 - slot_N(s)                                      # dense order: lbd0 first, no terminal slot
    wd = np.concatenate([w[w.size - nc0:], w[:body]])
    (torch.tensor(wd, dtype=torch.float64) * z).sum().backward()
    G = prob.copy()
    g = lambda tns, like: np.zeros_like(like) if tns.grad is None else tns.grad.numpy()
    for k, m in zip(G.stages, L):
        for name in m:
            getattr(k, name)[...] = g(m[name], getattr(k, name))
    G.G0[...], G.g0[...] = g(G0, prob.G0), g(g0, prob.g0)
    zn = z.detach().numpy()
    zvec = np.concatenate([zn[nc0:], np.zeros(slot_N(s)), zn[:nc0]])
    # the premise: numpy's dense KKT solve (oracle/dense_kkt.py) and the torch assembly agree on the solution
    ref = sol_to_vec(s, dense_kkt.dense_solve(prob, mueq))
    assert np.abs(zvec - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max()), np.abs(zvec - ref).max()
    return s.pack(G), zvec


def assert_autograd(s, probs, w, grad, mueq, label="", only=None):
    """the gradient records against autograd, the bar from the numpy formula on the oracle's solution and adjoint"""
    for b in (range(s.batch) if only is None else only):
        auto, _ = autograd_record(s, probs[b], w[b])
        z = sol_to_vec(s, pc.oracle_serial(probs[b], mueq)[2])
        d = sol_to_vec(s, pc.oracle_serial(with_affine(s, probs[b], w[b]), mueq)[2])
        e_ref = float(np.abs(formula(s, probs[b], z, d)[0] - auto).max())
        bar = max(1e-11 * float(np.abs(auto).max()), 10.0 * e_ref)
        err = float(np.abs(grad[b] - auto).max())
        print(f"adjoint {label} b={b}: gradient against autograd {err:.3e}, the oracle's formula {e_ref:.3e}, bar {bar:.3e}, "
              f"ratio {err / bar:.3f}, largest entry {np.abs(auto).max():.3e}")
        WORST["autograd"] = max(WORST["autograd"], err / bar)
        assert np.isfinite(grad[b]).all() and err <= bar, (label, b, err, bar)
    report()


# ---- device buffers ----------------------------------------------------------------------------------------------------------
class DevArray:
    """n doubles of device memory (the emulator's device memory is host memory)"""

    def __init__(self, n, lib_path, init=None):
        arr = np.zeros(n) if init is None else np.ascontiguousarray(init, dtype=np.float64).reshape(-1)
        self.n, self.lib_path = arr.size, lib_path
        self.keep, self.ptr = ac.to_device(arr, lib_path)

    def read(self):
        return kc.read_device(self.ptr, self.n, self.lib_path)


def raw_adjoints(s, lib_path):
    return kc.read_device(s.device_adjoints(), s.batch * s.device_solution_doubles, lib_path).reshape(s.batch, -1)


def everything(s, probs, mueq, lib_path, rng, label, formula_only=False, **opts):
    """one adjoint of the solved batch in s: d against the oracle, the records against the formula, the vectors of
    solution_vectors_device against solution(b).  -> (cot, adj, grad)"""
    cot = cotangents(s, rng)
    adj, grad = s.adjoint(cot)
    assert grad.shape == (s.batch, s.problem_doubles)
    if not formula_only:
        assert_adjoint(s, probs, cot, adj, mueq, lib_path, label=label, **opts)
    assert_formula(s, probs, adj, grad, label=label)
    out = DevArray(s.batch * s.affine_doubles, lib_path)
    s.solution_vectors_device(out.ptr)
    s.sync()
    vec = out.read().reshape(s.batch, -1)
    for b in range(s.batch):
        assert np.array_equal(bits(vec[b]), bits(sol_to_vec(s, s.solution(b)))), (label, b)
    adj_only, none = s.adjoint(cot, want_grad=False)
    assert none is None and np.array_equal(bits(adj_only), bits(adj))
    return cot, adj, grad


def end_to_end(probs, mueq, lib_path, rng, label, **opts):
    """generator "W" problems through upload_packed_user_device: the round trip, then the gradient against autograd"""
    s = kc.solver_for(probs, lib_path, **opts)
    packed = np.concatenate([s.pack(p) for p in probs])
    src = DevArray(packed.size, lib_path, packed)
    with kc.options(**opts):
        fresh = BatchedRiccatiSolver(s.dims, s.nc0, batch=s.batch, lib_path=lib_path)
    assert fresh.kernel_name == s.kernel_name
    fresh.upload_packed_user_device(src.ptr)
    fresh.sync()
    assert np.array_equal(bits(fresh.download_packed()), bits(packed)), label
    assert fresh.backward(mueq) and fresh.forward()
    w = cotangents(fresh, rng)
    adj, grad = fresh.adjoint(w)
    assert_autograd(fresh, probs, w, grad, mueq, label=label)
    assert s.backward(mueq) and s.forward()                       # the host upload gives the same bits
    adj2, grad2 = s.adjoint(w)
    assert np.array_equal(bits(adj), bits(adj2)) and np.array_equal(bits(grad), bits(grad2))
    return fresh


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def check_serial(lib_path, nx, nu, N, batch, kernel, mueq=1e-10, **opts):
    """a serial family: mode "F" problems against the oracle and the formula, mode "W" problems against autograd"""
    probs = rc.singular_problems(nx, nu, N, batch)
    s = rc.solved(probs, lib_path, mueq, **opts)
    assert s.kernel_name == kernel, s.kernel_name
    everything(s, probs, mueq, lib_path, np.random.default_rng([81, nx, nu]), kernel, **opts)
    end_to_end(kc.unconstrained(nx, nu, N, batch, seed=8), mueq, lib_path, np.random.default_rng([82, nx, nu]), kernel, **opts)


def check_padded(lib_path, nx, nu, N, kernel, mueq=1e-10):
    """the caller's dimensions on a padded solver; the dummy entries of the adjoint record in HBM are exactly zero"""
    probs = rc.singular_problems(nx, nu, N, 2)
    s = rc.solved(probs, lib_path, mueq, BACKWARD="wave")
    assert s.padded and s.kernel_name == kernel, (s.padded, s.kernel_name)
    _, adj, _ = everything(s, probs, mueq, lib_path, np.random.default_rng([83, nx, nu]), f"padded {kernel}", BACKWARD="wave")
    rec = raw_adjoints(s, lib_path)
    NX, NU = int(s.device_dims[0, 0]), int(s.device_dims[0, 1])
    for t in range(N + 1):
        x, u, l = (int(s.device_stage_offsets[t, c]) for c in (2, 3, 5))
        assert (rec[:, x + nx:x + NX] == 0.0).all(), t
        assert (rec[:, l + nx:l + NX] == 0.0).all(), t
        if t < N:
            assert (rec[:, u + nu:u + NU] == 0.0).all(), t
        assert np.array_equal(bits(rec[:, x:x + nx]), bits(np.stack([vec_to_sol(s, a)[0][t] for a in adj]))), t
    end_to_end(kc.unconstrained(nx, nu, N, 2, seed=9), mueq, lib_path, np.random.default_rng([84, nx, nu]), f"padded {kernel}",
               BACKWARD="wave")


def check_initial(lib_path, frac, kind, init, nx=8, nu=4, N=3, mueq=1e-10):
    """nc0 in {0, nx / 2, nx}, G0 = -I, +I, general, GAR_HIP_INIT unset and = bk: dG0 and dg0 are part of both records"""
    nc0 = {0: 0, 1: nx // 2, 2: nx}[frac]
    rng = np.random.default_rng([85, frac, isc.G0_KINDS.index(kind)])
    opts = dict(BACKWARD="wave")
    if init:
        opts["INIT"] = init
    probs = [isc.set_initial(p, nc0, kind, rng) for p in rc.singular_problems(nx, nu, N, 2)]
    s = rc.solved(probs, lib_path, mueq, **opts)
    assert s.kernel_name == f"wave<{nx},{nu}>", s.kernel_name
    label = f"init nc0={nc0} G0={kind} INIT={init}"
    _, adj, grad = everything(s, probs, mueq, lib_path, rng, label, **opts)
    if nc0:
        G = s.unpack_gradient(grad[0])
        assert np.abs(G.G0).max() > 0 and np.array_equal(bits(G.g0), bits(adj[0][-nc0:]))
    wprobs = [isc.set_initial(p, nc0, kind, rng) for p in kc.unconstrained(nx, nu, N, 2, seed=10)]
    end_to_end(wprobs, mueq, lib_path, rng, label, **opts)


def check_terminal(lib_path, which, mueq=1e-10):
    """a terminal knot with nx2 = 0, one knot (N = 0), a terminal knot with nu > 0 (generator "W": all three yardsticks)"""
    probs = ac.terminal_problems(which)
    s = rc.solved(probs, lib_path, mueq)
    rng = np.random.default_rng(86)
    _, _, grad = everything(s, probs, mueq, lib_path, rng, f"terminal {which}")
    G = s.unpack_gradient(grad[0]).stages[-1]
    assert not G.A.any() and not G.B.any() and not G.f.any()
    end_to_end(probs, mueq, lib_path, rng, f"terminal {which}")


def check_ring(lib_path, family, mueq=1e-10):
    """after two cycleAppends (a ring: no record moves): the records follow the caller's turned layout"""
    nx, nu, N = 8, 4, 5
    probs = rc.singular_problems(nx, nu, N, 2)
    rng = np.random.default_rng(87)
    s = rc.solved(probs, lib_path, mueq, BACKWARD=family)
    for _ in range(2):
        s.cycle_append(probs[0].stages[0].dims)
        with pytest.raises(RuntimeError, match="gar_hip error -1.*cycle_append"):
            s.adjoint(cotangents(s, rng))
        for b, p in enumerate(probs):
            new = synth.generate_knot(rng, nx, nu, mode="F")
            p.stages[:N] = p.stages[1:N] + [new]
            s.upload_knot(b, N - 1, new)
    assert int(s.stage_offsets[0, 0]) != int(s.stage_offsets[:, 0].min())      # the ring has turned
    assert s.backward(mueq) and s.forward()
    cot = cotangents(s, rng)
    adj, grad = s.adjoint(cot)
    sub = [with_affine(s, p, c) for p, c in zip(probs, cot)]
    full = rc.solved(sub, lib_path, mueq, BACKWARD=family)      # (a fresh solver of the same family: its ring has not turned)
    for b in range(2):
        ref = sol_to_vec(s, pc.oracle_serial(sub[b], mueq)[2])
        ratio = vec_distance(adj[b], ref) / max(vec_distance(sol_to_vec(s, full.solution(b)), ref), EPS)
        print(f"adjoint ring {family} b={b}: ratio {ratio:.3f}")
        WORST["adjoint"] = max(WORST["adjoint"], ratio)
        assert ratio <= MARGIN
    assert_formula(s, probs, adj, grad, label=f"ring {family}")
    src = DevArray(s.batch * s.problem_doubles, lib_path, s.download_packed())
    before = s.download_packed()
    s.upload_packed_user_device(src.ptr)
    s.sync()
    assert np.array_equal(bits(before), bits(s.download_packed()))


def check_grid(lib_path, mueq=1e-10):
    """70 problems of (8, 4), N = 2: each problem's gradient equals its batch-1 gradient, bitwise"""
    probs = rc.singular_problems(8, 4, 2, 70)
    s = rc.solved(probs, lib_path, mueq, BACKWARD="wave")
    cot = cotangents(s, np.random.default_rng(88))
    adj, grad = s.adjoint(cot)
    one = kc.solver_for(probs[:1], lib_path, BACKWARD="wave")
    for b in range(70):
        one.upload(probs[b:b + 1])
        assert one.backward(mueq) and one.forward()
        a1, g1 = one.adjoint(cot[b:b + 1])
        assert np.array_equal(bits(a1[0]), bits(adj[b])) and np.array_equal(bits(g1[0]), bits(grad[b])), b
    assert_formula(s, probs, adj, grad, label="grid", only=(0, 33, 69))


def snapshot(s, lib_path):
    pe, ps = s.device_kkt_errors()
    kkt = [kc.read_device(pe, s.batch * 3, lib_path), kc.read_device(ps, s.batch * (s.horizon + 1) * 4, lib_path)] if pe else []
    return [rc.raw_knots(s, lib_path), s.download_packed(), ac.raw_factors(s, lib_path), ac.raw_solutions(s, lib_path),
            s.status().astype(np.float64)] + kkt + rc.gains_and_values(s)


def check_untouched(lib_path, family, mueq=1e-10):
    """the adjoint writes nothing of the primal; a refine(1) before and after it gives the bits it gives without it.
    W = R-hat^-1 has no accessor: it is held through that refinement step, whose sweep multiplies by every entry of W --
    the solution and the KKT triples after it equal, bitwise, those of a solver that ran no adjoint"""
    nx, nu, N = 8, 4, 4
    probs = rc.singular_problems(nx, nu, N, 3)
    rng = np.random.default_rng(89)
    s, plain = rc.solved(probs, lib_path, mueq, BACKWARD=family), rc.solved(probs, lib_path, mueq, BACKWARD=family)
    cot = cotangents(s, rng)
    for q in (s, plain):
        assert q.refine(1) == (1, 3)                  # (W and the KKT buffers exist from here on)
    before = snapshot(s, lib_path)
    adj, grad = s.adjoint(cot)
    out, dcot = DevArray(s.batch * s.problem_doubles, lib_path), DevArray(cot.size, lib_path, cot)
    s.adjoint_async(dcot.ptr, 0, out.ptr)
    s.sync()
    assert np.array_equal(bits(out.read()), bits(grad.ravel()))
    after = snapshot(s, lib_path)
    assert len(before) == len(after) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, after))
    for q in (s, plain):
        assert q.refine(1) == (1, 3)
    assert np.array_equal(bits(ac.raw_solutions(s, lib_path)), bits(ac.raw_solutions(plain, lib_path)))
    assert np.array_equal(bits(kc.device_results(s, lib_path)[0]), bits(kc.device_results(plain, lib_path)[0]))
    adj2, grad2 = s.adjoint(cot)                      # ... and the adjoint follows the refined solution
    assert np.array_equal(bits(adj), bits(adj2)) and not np.array_equal(bits(grad), bits(grad2))


def check_failed_problem(lib_path, mueq=1e-8):
    """problem 1 of three fails its backward: zero records for it, the others as in a batch without it"""
    nx, nu, N = 8, 4, 5
    probs = rc.singular_problems(nx, nu, N, 3)
    good = [p.copy() for p in probs]
    bad = probs[1].stages[2]
    bad.R[...] = 0.0
    bad.S[...] = 0.0
    bad.B[...] = 0.0
    s = kc.solver_for(probs, lib_path, BACKWARD="wave")
    pc.assert_reported_failure(s.backward, mueq)
    assert [bool(v) for v in s.status()] == [False, True, False]
    s.forward()
    cot = cotangents(s, np.random.default_rng(90))
    dcot, dadj, dgrad = (DevArray(a.size, lib_path, a) for a in (cot, np.ones(cot.size), np.ones(3 * s.problem_doubles)))
    s.adjoint_async(dcot.ptr, dadj.ptr, dgrad.ptr)                # (the asynchronous form does not wait: no report)
    s.sync()
    adj, grad = dadj.read().reshape(3, -1), dgrad.read().reshape(3, -1)
    assert not adj[1].any() and not grad[1].any() and not raw_adjoints(s, lib_path)[1].any()
    with pytest.raises(RuntimeError, match="Failed stage LDL factorization"):
        s.adjoint(cot)
    ok = rc.solved(good, lib_path, mueq, BACKWARD="wave")
    adj_ok, grad_ok = ok.adjoint(cot)
    for b in (0, 2):
        assert np.array_equal(bits(adj[b]), bits(adj_ok[b])) and np.array_equal(bits(grad[b]), bits(grad_ok[b])), b
    assert [bool(v) for v in s.status()] == [False, True, False] and s.num_failed() == 1


def both_forms(s, lib_path):
    cot = np.ones((s.batch, max(s.affine_doubles, 1)))
    dcot = DevArray(cot.size, lib_path, cot)
    dadj, dgrad = DevArray(cot.size, lib_path), DevArray(s.batch * s.problem_doubles, lib_path)

    def async_form():
        try:
            s.adjoint_async(dcot.ptr, dadj.ptr, dgrad.ptr)
        finally:
            s.sync()
            assert not dadj.read().any() and not dgrad.read().any()        # nothing written
    return (lambda: s.adjoint(cot), async_form, lambda: s.adjoint(cot, want_grad=False))


def check_refusals(lib_path, what, devices=(0, 0), mueq=1e-6):
    """the unserved kinds answer GAR_HIP_ERR_UNSUPPORTED; no backward, no forward, a null cotangent GAR_HIP_ERR_ARG"""
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
        return rc.untouched_by(s, lib_path, both_forms(s, lib_path), -1, "no backward")
    elif what == "no forward":
        s = rc.solved(kc.unconstrained(nx, nu, N, 2), lib_path, mueq)
        assert s.backward(mueq)
        rc.untouched_by(s, lib_path, both_forms(s, lib_path), -1, "no forward")
        assert s.forward() and np.isfinite(s.adjoint(np.ones((2, s.affine_doubles)))[1]).all()
        return
    else:                                   # a null cotangent
        s = rc.solved(kc.unconstrained(nx, nu, N, 2), lib_path, mueq)
        dgrad = DevArray(2 * s.problem_doubles, lib_path)
        calls = (lambda: s._check(s._L.gar_hip_adjoint(s._h, None, None, None)), lambda: s.adjoint_async(0, 0, dgrad.ptr))
        rc.untouched_by(s, lib_path, calls, -1, "null cotangent")
        assert not dgrad.read().any()
        return
    src = DevArray(s.batch * s.problem_doubles, lib_path)
    out = DevArray(s.batch * max(s.affine_doubles, 1), lib_path)
    rc.untouched_by(s, lib_path, both_forms(s, lib_path) + (lambda: s.upload_packed_user_device(src.ptr),
                                                            lambda: s.solution_vectors_device(out.ptr)), -3)
    assert not out.read().any()


def check_allocation(lib_path, rounds=20, mueq=1e-10):
    """the first calls may allocate; twenty further rounds do not, a backward and a refine in between included"""
    L = _lib.load(lib_path)
    probs = rc.singular_problems(8, 4, 3, 3)
    s = rc.solved(probs, lib_path, mueq)
    assert s.refine(1) == (1, 3)        # (the KKT buffers, the re-solve's and the refinement's side buffers exist from here on)
    cot = cotangents(s, np.random.default_rng(91))
    dcot, dadj, dgrad = DevArray(cot.size, lib_path, cot), DevArray(cot.size, lib_path), DevArray(3 * s.problem_doubles, lib_path)
    c0 = L.gar_hip_debug_alloc_count()
    s.adjoint(cot)
    s.adjoint_async(dcot.ptr, dadj.ptr, dgrad.ptr)
    s.sync()
    c1 = L.gar_hip_debug_alloc_count()
    assert 0 < c1 - c0 <= 4             # the adjoint records and gate words (2), the host form's staging (2)
    for i in range(rounds):
        s.adjoint(cot)
        s.adjoint_async(dcot.ptr, dadj.ptr, dgrad.ptr)
        s.adjoint(cot, want_grad=False)
        if i == rounds // 2:
            assert s.backward(mueq) and s.forward() and s.refine(1) == (1, 3)
    s.sync()
    assert L.gar_hip_debug_alloc_count() == c1


def check_no_host_sync(lib_path, mueq=1e-10, pipeline=False):
    """upload_packed_user_device -> backward_async -> forward_async -> solution_vectors_device -> adjoint_async -> sync:
    bitwise what the synchronous calls give"""
    probs = rc.singular_problems(8, 4, 5, 5)
    s, ref = kc.solver_for(probs, lib_path, BACKWARD="wave"), kc.solver_for(probs, lib_path, BACKWARD="wave")
    if pipeline:
        for q in (s, ref):
            q.set_pipeline(2)
            assert q.pipeline == 2
    cot = cotangents(s, np.random.default_rng(92))
    packed = np.concatenate([s.pack(p) for p in probs])
    src, dcot = DevArray(packed.size, lib_path, packed), DevArray(cot.size, lib_path, cot)
    dsol, dadj, dgrad = DevArray(cot.size, lib_path), DevArray(cot.size, lib_path), DevArray(packed.size, lib_path)
    s.upload_packed_user_device(src.ptr)
    s.backward_async(mueq)
    s.forward_async()
    s.solution_vectors_device(dsol.ptr)
    s.adjoint_async(dcot.ptr, dadj.ptr, dgrad.ptr)
    s.sync()
    assert s.num_failed() == 0
    assert ref.backward(mueq) and ref.forward()
    adj, grad = ref.adjoint(cot)
    assert np.array_equal(bits(dadj.read()), bits(adj.ravel())) and np.array_equal(bits(dgrad.read()), bits(grad.ravel()))
    assert np.array_equal(bits(dsol.read()), bits(np.concatenate([sol_to_vec(ref, ref.solution(b)) for b in range(5)])))
    label = "no host sync" + (" (pipelined)" if pipeline else "")
    assert_adjoint(s, probs, cot, adj, mueq, lib_path, label=label, BACKWARD="wave")
    assert_formula(s, probs, adj, grad, label=label)


def check_invalidation(lib_path, mueq=1e-10):
    """new matrices through upload_packed_user_device refuse the adjoint until the next backward"""
    nx, nu, N = 8, 4, 4
    probs, others = rc.singular_problems(nx, nu, N, 2), kc.unconstrained(nx, nu, N, 2, seed=11)
    s = rc.solved(probs, lib_path, mueq, BACKWARD="wave")
    rng = np.random.default_rng(93)
    everything(s, probs, mueq, lib_path, rng, "before new matrices", formula_only=True)
    src = DevArray(2 * s.problem_doubles, lib_path, np.concatenate([s.pack(p) for p in others]))
    s.upload_packed_user_device(src.ptr)
    s.sync()
    rc.untouched_by(s, lib_path, both_forms(s, lib_path), -1, r"\(gar_hip_upload_packed_user_device\)")
    rc.untouched_by(s, lib_path, rc.both_forms(s), -1, r"\(gar_hip_upload_packed_user_device\)")
    assert s.backward(mueq) and s.forward()
    everything(s, others, mueq, lib_path, rng, "after new matrices (a stale W fails here)", BACKWARD="wave")


def check_round_trip(lib_path, kind):
    """upload_packed_user_device then download_packed: the caller's packed problems, bitwise; the device knots equal those
    of the host upload"""
    nx, nu, N, opts = {"plain": (8, 4, 3, dict(BACKWARD="wg4")), "qr-packed": (36, 12, 2, dict(BACKWARD="wave")),
                       "padded": (4, 2, 3, dict(BACKWARD="wave"))}[kind]
    probs = kc.unconstrained(nx, nu, N, 3, seed=12)
    if kind != "qr-packed":                         # a general G0 with fewer rows than states
        probs = [isc.set_initial(p, nx // 2, "gen", np.random.default_rng(94)) for p in probs]
    s, host = kc.solver_for(probs, lib_path, **opts), kc.solver_for(probs, lib_path, **opts)
    assert s.padded == (kind == "padded") and s.qr_packed == (kind == "qr-packed" or (s.padded and s.qr_packed)), \
        (s.kernel_name, s.padded, s.qr_packed)
    packed = np.concatenate([s.pack(p) for p in probs])
    src = DevArray(packed.size, lib_path, packed[s.problem_doubles:])
    with kc.options(**opts):
        fresh = BatchedRiccatiSolver(s.dims, s.nc0, batch=3, lib_path=lib_path)
    fresh.upload_packed_user_device(DevArray(s.problem_doubles, lib_path, packed[:s.problem_doubles]).ptr, 0, 1)
    fresh.upload_packed_user_device(src.ptr, 1, 2)
    fresh.sync()
    assert np.array_equal(bits(fresh.download_packed()), bits(packed))
    assert fresh.backward(1e-10) and fresh.forward() and host.backward(1e-10) and host.forward()
    assert np.array_equal(bits(rc.raw_knots(fresh, lib_path)), bits(rc.raw_knots(host, lib_path)))
    assert np.array_equal(bits(ac.raw_solutions(fresh, lib_path)), bits(ac.raw_solutions(host, lib_path)))


def check_layer(lib_path, device, mueq=1e-10):
    """LqLayer on (8, 4), N = 5, batch 3: packed.grad against autograd; a second round on the same layer, bitwise a fresh one"""
    import torch
    from aligator_amd.layer import LqLayer
    nx, nu, N = 8, 4, 5
    rng = np.random.default_rng(95)

    def round_of(layer, probs, w):
        s = layer.solver
        packed = torch.tensor(np.stack([s.pack(p) for p in probs]), dtype=torch.float64, device=device, requires_grad=True)
        out = layer(packed)
        (torch.tensor(w, dtype=torch.float64, device=device) * out).sum().backward()
        if device != "cpu":
            torch.cuda.synchronize()
        s.sync()
        assert not s.status().any()
        return out.detach().cpu().numpy(), packed.grad.detach().cpu().numpy()

    def new_layer(probs):
        with kc.options(BACKWARD="wave"):
            return LqLayer(BatchedRiccatiSolver([k.dims for k in probs[0].stages], probs[0].nc0, batch=3, lib_path=lib_path), mueq)

    first, second = kc.unconstrained(nx, nu, N, 3, seed=13), kc.unconstrained(nx, nu, N, 3, seed=14)
    layer = new_layer(first)
    s = layer.solver
    w = cotangents(s, rng)
    out, grad = round_of(layer, first, w)
    for b in range(3):
        assert np.array_equal(bits(out[b]), bits(sol_to_vec(s, s.solution(b))))
    assert_autograd(s, first, w, grad, mueq, label=f"layer on {device}")
    packed = torch.tensor(np.stack([s.pack(p) for p in first]), dtype=torch.float64, device=device, requires_grad=True)
    stale = layer(packed).sum()
    layer(packed.detach())                           # the solver moves on: the first graph no longer matches what it holds
    with pytest.raises(RuntimeError, match="another forward"):
        stale.backward()
    out2, grad2 = round_of(layer, second, w)
    out3, grad3 = round_of(new_layer(second), second, w)
    assert np.array_equal(bits(out2), bits(out3)) and np.array_equal(bits(grad2), bits(grad3))
    assert_autograd(s, second, w, grad2, mueq, label=f"layer on {device}, second round")
