"""The initial stage (proximal-riccati.hxx:42-60: factorise kkt0 = [Vxx0 G0^T; G0 0], solve for [x0; lambda0]) over what
a caller may hand it: nc0 from 0 to nx, G0 = -I, +I or general, and GAR_HIP_INIT=bk (which keeps the factorisation for
every G0) -- cases and checks shared by the emulator tests (tests/test_init_stage.py) and the GPU tests
(tests/test_init_stage_gpu.py).  DESIGN.md section 2 lists which implementation of the initial stage each kernel family
runs; every row below names the family it must bind (kernel_name), so that no row falls onto the any-dimension kernels
unnoticed.

Every case first checks its premises on the reference side alone (premises()): which kinds are eligible for the closed
form, that the oracle solves the problem, and that the oracle and LAPACK agree on it to 1e-10.  Then the library is held
to the checks of parity_cases (solution, every factor block, kkt0.ff / fth, thGrad, thHess, KKT residual) at 1e-9 on
generator "W", and -- the oracle restates the same algorithm -- to the 50-digit solutions of
tests/golden/init/initial_stage.npz (row X1)."""
import importlib.util
import os

import numpy as np

from aligator_amd import synth
from aligator_amd.gar import lqrComputeKktError, lqrInitializeSolution
from aligator_amd.lqr import LqrProblem
import parity_cases as pc
import serial_fold_cases as sf

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "init", "initial_stage.npz")

G0_KINDS = ("-I", "+I", "gen")
# kind -> (nc0 of an nx-dimensional initial state, G0)
KINDS = {
    "K0": (lambda nx: 0, None),                        # free initial state
    "K1": (lambda nx: max(1, nx // 3), "gen"),
    "K2": (lambda nx: nx - 1, "-I"),                   # rows of -I: must NOT take the closed form
    "K3": (lambda nx: nx, "+I"),                       # closed form, s = +1
    "K4": (lambda nx: nx, "gen"),
    "K5": (lambda nx: nx, "-I"),                       # closed form, s = -1: what every other test sweeps
}
ALL_KINDS = tuple(KINDS)
LEG_KINDS = ("K0", "K1", "K3", "K4")
INITS = (None, "bk")                                   # GAR_HIP_INIT: unset (closed form where eligible), "bk"
UNCONSTRAINED_AGREEMENT = 1e-10                        # oracle against LAPACK on every unconstrained case


def init_id(init):
    return "default" if init is None else init


def set_initial(prob, nc0, g0kind, rng):
    """The same knots under another initial condition: nc0 rows, g0 = randn, G0 by kind with E = eye(nc0, nx)."""
    nx = prob.stages[0].nx
    out = LqrProblem(prob.stages, nc0)
    if nc0:
        E = np.eye(nc0, nx)
        if g0kind == "-I":
            out.G0[...] = -E
        elif g0kind == "+I":
            out.G0[...] = E
        elif g0kind == "gen":          # (a fully random square G0 drives |lambda0| to 1e6: nothing left to compare)
            out.G0[...] = -E + 0.2 * rng.standard_normal((nc0, nx))
        else:
            raise ValueError(g0kind)
        out.g0[...] = rng.standard_normal(nc0)
    return out


def problem(nx, nu, N, nc0, kind, nc=0, nth=0, seed=0, mode="W", random_D=False):
    """The stages of synth.generate_lq_problem(..., mode) under the initial condition (nc0, kind), kind one of
    G0_KINDS (ignored at nc0 = 0).  random_D: a random D on every knot that has controls."""
    rng = np.random.default_rng([seed, nx, nu, N, nc0, nc, nth, G0_KINDS.index(kind) if nc0 else 3])
    base = synth.generate_lq_problem(rng, np.zeros(nx), N, nx, nu, nth=nth, nc=nc, mode=mode)
    if random_D:
        for k in base.stages[:-1]:
            k.D[...] = rng.uniform(-1, 1, k.D.shape)
    return set_initial(base, nc0, kind, rng)


def kind_problem(kind, nx, nu, N, **kw):
    nc0, g0kind = KINDS[kind]
    return problem(nx, nu, N, nc0(nx), g0kind or "-I", **kw)


def heterogeneous_problem(kind, seed=8):
    """nx, nu vary along the horizon (the emulator's test_heterogeneous_dimensions): nx0 = 3 differs from later nx."""
    rng = np.random.default_rng([seed, ALL_KINDS.index(kind)])
    shapes = [(3, 2, 4), (4, 1, 5), (5, 3, 2), (2, 2, 2)]     # (nx, nu, nx2)
    knots = [synth.generate_knot(rng, nx, nu, nx2=nx2, mode="W") for nx, nu, nx2 in shapes]
    knots.append(synth.generate_knot(rng, 2, 0, mode="W"))
    nc0, g0kind = KINDS[kind]
    return set_initial(LqrProblem(knots, 0), nc0(3), g0kind, rng)


def is_plus_minus_identity(G0, nx):
    return G0.shape == (nx, nx) and (np.array_equal(G0, np.eye(nx)) or np.array_equal(G0, -np.eye(nx)))


_PREMISES = {}


def premises(key, prob, kind, mueq):
    """On the reference alone, once per problem: the closed form is eligible for K3 / K5 and for no other kind; the
    reference solves the problem; without constraints the oracle and LAPACK agree on it to 1e-10."""
    if key in _PREMISES:
        return _PREMISES[key]
    nx = prob.stages[0].nx
    assert prob.nc0 == KINDS[kind][0](nx), (prob.nc0, kind)
    assert is_plus_minus_identity(np.asarray(prob.G0), nx) == (kind in ("K3", "K5")), kind
    assert pc.reference_solvable(prob, mueq), key
    worst = None
    if not any(k.nc > 0 for k in prob.stages):
        bound, _ = pc.conditioning_bound(prob, mueq)
        worst = max(bound)
        assert worst <= UNCONSTRAINED_AGREEMENT, (key, bound)
    _PREMISES[key] = worst
    return worst


def rel_error(sol, ref):
    return max(pc.maxdiff(A, B) for A, B in zip(sol, ref)) / pc.scale_of(ref)


# ---- serial rows -----------------------------------------------------------------------------------------------------
def _srow(shape, N, kernel, what, opts=None, mueq=1e-10, kinds=ALL_KINDS, mode="W", tol=1e-9, dense=False, parity=False,
          seed=0):
    return dict(shape=shape, N=N, kernel=kernel, what=what, opts=opts or {}, mueq=mueq, kinds=kinds, mode=mode, tol=tol,
                dense=dense, parity=parity, seed=seed)


# shape = (nx, nu, nc, nth); parity: also at N = 1 and N = 2 with K1 (the hand-off from the last stage into the tail at
# both parities of the horizon)
SERIAL_ROWS = {
    "S1": _srow((36, 12, 0, 0), 3, "wave<36,12>", "fused tail, packed Bunch-Kaufman up to n0 = 72",
                opts={"BACKWARD": "wave"}, parity=True),
    "S2": _srow((36, 12, 0, 0), 3, "mfma<36,12>", "gar_initial_wave on the packed Vxx record",
                opts={"BACKWARD": "wg4"}, parity=True),
    "S3": _srow((5, 2, 0, 0), 3, "wave<8,4>", "padded: set_init's [G0 0; 0 -I], nc0 = user + 3",
                opts={"BACKWARD": "wave"}),
    "S4": _srow((36, 12, 32, 0), 3, "wave<36,12,32>", "fused tail behind the constrained chain", mueq=1e-6,
                parity=True),
    "S5": _srow((56, 24, 0, 0), 2, "pair<56,24>", "gar_initial_wave at n0 = 56 ... 112", parity=True, seed=1),
    "S6": _srow((10, 4, 0, 2), 5, "generic", "workgroup initial_stage with theta columns"),
    "S7": _srow((6, 3, 2, 2), 4, "dense", "the stage-dense solver's initial stage", mueq=1e-6, dense=True),
    "S8": _srow(None, 4, "generic", "nx0 differs from later nx"),
    "S9": _srow((6, 2, 3, 3), 4, "generic", "parameters and constraints (generator F)", mueq=1e-9, kinds=("K1", "K5"),
                mode="F", tol=1e-8),
}


def serial_cases():
    """(row, kind, init, N) of every serial case"""
    out = []
    for name, r in SERIAL_ROWS.items():
        out += [(name, kind, init, r["N"]) for kind in r["kinds"] for init in INITS]
        if r["parity"]:
            out += [(name, "K1", init, N) for N in (1, 2) if N != r["N"] for init in INITS]
    return out


def serial_problem(row, kind, N):
    r = SERIAL_ROWS[row]
    if r["shape"] is None:
        return heterogeneous_problem(kind), None
    nx, nu, nc, nth = r["shape"]
    prob = kind_problem(kind, nx, nu, N, nc=nc, nth=nth, mode=r["mode"], seed=r["seed"])
    theta = np.random.default_rng([7, nx, nth]).uniform(-1, 1, nth) if nth else None
    return prob, theta


def check_serial_case(row, kind, init, N, lib_path=None):
    """-> the largest relative error of the solution against the oracle"""
    r = SERIAL_ROWS[row]
    prob, theta = serial_problem(row, kind, N)
    premises((row, kind, N), prob, kind, r["mueq"])
    constrained = any(k.nc > 0 for k in prob.stages)
    with sf.options(INIT=init, **r["opts"]):
        if r["dense"]:
            s, sol, ref = pc.check_dense(prob, r["mueq"], r["tol"], lib_path, theta=theta, conditioned=constrained)
        else:
            s, sol, ref = pc.check_serial(prob, r["mueq"], r["tol"], lib_path, theta=theta, conditioned=constrained,
                                          conditioned_factors=constrained)
    assert s.kernel_name == r["kernel"], (s.kernel_name, r["kernel"])
    assert s._impl.num_failed() == 0 and not s._impl.status().any()
    assert_kkt(prob, sol, ref, r["mueq"], r["tol"], theta)
    return rel_error(sol, ref)


def assert_kkt(prob, sol, ref, mueq, tol, theta=None):
    """The KKT residual relative to the solution's scale: tol, and on a constrained problem no less than
    CONDITIONING_MARGIN x the oracle's own residual (the rule of parity_cases.check_mueq_case)."""
    sc = pc.scale_of(ref)
    kkt = max(lqrComputeKktError(prob, *sol, mueq=mueq, theta=theta)) / sc
    bar = tol
    if any(k.nc > 0 for k in prob.stages):
        bar = max(tol, pc.CONDITIONING_MARGIN * max(lqrComputeKktError(prob, *ref, mueq=mueq, theta=theta)) / sc)
    assert kkt <= bar, (kkt, bar)


# ---- leg mode --------------------------------------------------------------------------------------------------------
def _lrow(shape, N, legs, kernel, opts=None, mueq=1e-10, random_D=False, condensed=None):
    return dict(shape=shape, N=N, legs=legs, kernel=kernel, opts=opts or {}, mueq=mueq, random_D=random_D,
                condensed=condensed)


GENERIC_LEGS = {"PAD": "0", "FORCE_GENERIC": "1"}
# shape = (nx, nu, nc)
LEG_ROWS = {
    "L1": _lrow((36, 12, 0), 9, 4, "wave_leg<36,12>"),
    "L2": _lrow((56, 24, 0), 7, 3, "pair_leg<56,24>"),
    "L3": _lrow((8, 4, 3), 11, 3, "wave_leg<8,4>+fold", mueq=1e-6),
    "L4": _lrow((8, 4, 4), 9, 3, "wave_leg<8,4>+fold|wave_seg<8,4,4>", mueq=1e-6, random_D=True),
    "L5": _lrow((5, 2, 0), 9, 3, "wave_leg<8,4>"),
    # the any-dimension leg kernels, the condensed system on gar_condensed_cr.hpp with a J that is no power of two
    "L6a": _lrow((9, 3, 0), 16, 8, "generic", opts=GENERIC_LEGS, condensed="reduced+cyclic"),
    "L6b": _lrow((6, 2, 0), 27, 13, "generic", opts=GENERIC_LEGS, condensed="reduced+cyclic"),
}


def leg_cases():
    return [(name, kind, init) for name in LEG_ROWS for kind in LEG_KINDS for init in INITS]


def check_leg_case(row, kind, init, lib_path=None):
    r = LEG_ROWS[row]
    nx, nu, nc = r["shape"]
    prob = kind_problem(kind, nx, nu, r["N"], nc=nc, random_D=r["random_D"], seed=ord(row[1]))
    premises((row, kind), prob, kind, r["mueq"])
    with sf.options(INIT=init, **r["opts"]):
        par = pc.check_parallel(prob, r["mueq"], r["legs"], 1e-9, lib_path, conditioned=nc > 0)
    assert par.kernel_name == r["kernel"], (par.kernel_name, r["kernel"])
    if r["condensed"]:
        assert par._impl.condensed_solver_name == r["condensed"], par._impl.condensed_solver_name
    assert par._impl.num_failed() == 0
    _, _, ref = pc.oracle_serial(prob, r["mueq"])
    return rel_error(par.checked_solution, ref)


# ---- batch and schedule ----------------------------------------------------------------------------------------------
BATCH_ROWS = ("S1", "S2", "S5")


def _against_oracle(s, probs, mueq, tol=1e-9):
    worst = 0.0
    for b, p in enumerate(probs):
        _, _, ref = pc.oracle_serial(p, mueq)
        sol = s.solution(b)
        worst = max(worst, rel_error(sol, ref))
        sc = pc.scale_of(ref)
        for A, B in zip(sol, ref):
            assert pc.maxdiff(A, B) <= tol * sc, b
    return worst


def check_mixed_batch(row, lib_path=None):
    """B1: one launch, nc0 = nx, G0 = (-I, gen, +I, gen).  The branch is taken per problem: problems 0 and 2 return
    x0 = -s g0 exactly (the closed form computes that and nothing else), the other two are factorised."""
    r = SERIAL_ROWS[row]
    nx, nu = r["shape"][:2]
    g0kinds = ("-I", "gen", "+I", "gen")
    probs = [problem(nx, nu, r["N"], nx, k, seed=40 + b) for b, k in enumerate(g0kinds)]
    for b, (p, k) in enumerate(zip(probs, g0kinds)):
        assert is_plus_minus_identity(np.asarray(p.G0), nx) == (k != "gen")
        premises((row, "B1", b), p, "K4" if k == "gen" else "K3", r["mueq"])
    with sf.options(INIT=None, **r["opts"]):
        s = sf.batched(probs, lib_path)
    assert s.kernel_name == r["kernel"], s.kernel_name
    assert s.backward(r["mueq"]) and s.forward()
    assert s.num_failed() == 0 and not s.status().any(), s.status()
    err = _against_oracle(s, probs, r["mueq"])
    for b, sgn in ((0, -1.0), (2, 1.0)):
        assert np.array_equal(s.solution(b)[0][0], -sgn * probs[b].g0), b
        assert np.array_equal(s.initial(b)[0][:nx], -sgn * probs[b].g0), b
    return err


PIPELINED = {"free": (0, "gen"), "partial": (12, "gen"), "plus_identity": (36, "+I")}


def _async_sweep(s, mueq, halves, steps):
    s.set_pipeline(halves)
    for _ in range(steps):
        s.backward_async(mueq)
        s.forward_async()
    s.sync()
    assert s.num_failed() == 0 and not s.status().any()
    return [[[a.copy() for a in part] for part in s.solution(b)] for b in range(s.batch)]


def check_pipelined(case, lib_path=None, mueq=1e-12):
    """B2: wave<36,12>, N = 4, a batch of 5 (uneven halves), two pipelined steps.  nc0 < nx never takes the closed form:
    every problem is handed to gar_initial_wave behind the sweep.  Against the oracle (1e-9), and against the plain
    schedule of the same solver (1e-11: the two factorise differently stored matrices; +I stays closed form in both
    schedules and is the same bits)."""
    nx, nu, N, batch = 36, 12, 4, 5
    nc0, g0kind = PIPELINED[case]
    probs = [problem(nx, nu, N, nc0, g0kind, seed=60 + b) for b in range(batch)]
    kind = {0: "K0", 12: "K1", 36: "K3"}[nc0]
    for b, p in enumerate(probs):
        premises(("B2", case, b), p, kind, mueq)
    with sf.options(INIT=None, BACKWARD="wave"):   # (a batch below the CU count would bind the 4-wave kernel)
        s = sf.batched(probs, lib_path)
    assert s.kernel_name == "wave<36,12>", s.kernel_name
    plain = _async_sweep(s, mueq, 0, 1)
    piped = _async_sweep(s, mueq, 2, 2)
    assert s.pipeline == 2
    err = _against_oracle(s, probs, mueq)
    worst = 0.0
    for b in range(batch):
        _, _, ref = pc.oracle_serial(probs[b], mueq)
        sc = pc.scale_of(ref)
        for A, B in zip(piped[b], plain[b]):
            d = pc.maxdiff(A, B)
            worst = max(worst, d / sc)
            assert d == 0.0 if g0kind == "+I" else d <= 1e-11 * sc, (b, d)
    s.close()
    return err, worst


def check_switch(row, kind, lib_path=None):
    """B3: GAR_HIP_INIT=bk has an effect where it should and none where it cannot.  K5: the default returns
    kkt0.ff[:nx] = g0 exactly (s = -1), the forced factorisation agrees with the oracle to 1e-9.  K1 / K2: the closed form
    is not eligible, both settings run the same code -- the same bits.  -> (error of the forced factorisation against
    the oracle, whether it reproduced x0 bit for bit: reported, not asserted)."""
    r = SERIAL_ROWS[row]
    nx, nu = r["shape"][:2]
    N, mueq = r["N"], r["mueq"]
    prob, _ = serial_problem(row, kind, N)
    premises((row, kind, N), prob, kind, mueq)
    solvers = {}
    for init in INITS:
        with sf.options(INIT=init, **r["opts"]):
            s = sf.batched([prob], lib_path)
        assert s.kernel_name == r["kernel"], s.kernel_name
        assert s.backward(mueq) and s.forward() and s.num_failed() == 0
        solvers[init] = s
    err = _against_oracle(solvers["bk"], [prob], mueq)
    same_x0 = np.array_equal(solvers[None].solution(0)[0][0], solvers["bk"].solution(0)[0][0])
    if kind == "K5":
        assert np.array_equal(solvers[None].initial(0)[0][:nx], prob.g0)
        _, osol, ref = pc.oracle_serial(prob, mueq)
        for s in solvers.values():
            ff = s.initial(0)[0]
            assert np.abs(ff - osol.kkt0_ff).max() <= 1e-9 * max(1.0, np.abs(osol.kkt0_ff).max())
        sc = pc.scale_of(ref)
        for A, B in zip(solvers[None].solution(0), solvers["bk"].solution(0)):
            assert pc.maxdiff(A, B) <= 1e-9 * sc
    else:
        assert kind in ("K1", "K2")
        sf.bitwise_equal(solvers[None], 0, solvers["bk"], 0, N)
    return err, same_x0


SERIAL_FOLD_KINDS = ("K0", "K1", "K4")


SERIAL_FOLD_FAMILIES = ("wave", "wg4")


def check_serial_fold(kind, init, lib_path=None, mueq=1e-6, family="wave"):
    """P1: the serial fold (GAR_HIP_SERIAL_FOLD=1) on case B of serial_fold_cases under another initial condition.  On
    `wave` the fused tail runs behind the sweep of the folded knots; on `wg4` the stand-alone initial stage reads stage 0's
    value function from the folded records (make_folded_params).  Held to the fold's own checks
    (serial_fold_cases.assert_parity)."""
    nx = sf.CASES["B"][0]
    nc0, g0kind = KINDS[kind]
    probs = [set_initial(p, nc0(nx), g0kind, np.random.default_rng([11, b, ALL_KINDS.index(kind)]))
             for b, p in enumerate(sf.make_batch("B"))]
    for b, p in enumerate(probs):
        premises(("P1", kind, b), p, kind, mueq)
    with sf.options(SERIAL_FOLD="1", BACKWARD=family, INIT=init):
        s = sf.batched(probs, lib_path)
    assert s.kernel_name == sf.fold_name("B", family), s.kernel_name
    assert s.backward(mueq) and s.forward()
    assert s.num_failed() == 0 and not s.status().any()
    sf.assert_parity(s, probs, mueq)
    worst = 0.0
    for b, p in enumerate(probs):
        _, _, ref = pc.oracle_serial(p, mueq)
        worst = max(worst, rel_error(s.solution(b), ref))
    return worst


# ---- the exact fixture -----------------------------------------------------------------------------------------------
GOLDEN_MUEQ = 1e-6
GOLDEN_FLOOR = 1e-11            # the floor MUEQ_GOLDEN_TOL uses on well-conditioned rows
# set -> (nx, nu, nc, N, kinds, random D)
GOLDEN_SETS = {
    "plain": (8, 4, 0, 5, ALL_KINDS, False),
    "padded": (5, 2, 0, 3, ALL_KINDS, False),
    "cstr": (8, 4, 4, 5, ("K0", "K1", "K4"), True),
}


def golden_problem(gset, kind):
    nx, nu, nc, N, _, rD = GOLDEN_SETS[gset]
    return kind_problem(kind, nx, nu, N, nc=nc, random_D=rD, seed=90)


def golden_keys():
    return [(g, kind) for g, v in GOLDEN_SETS.items() for kind in v[4]]


def golden_problems():
    return {f"{g}_{kind}": golden_problem(g, kind) for g, kind in golden_keys()}


_GOLDEN = {}


def load_golden():
    """{set_kind: [xs, us, vs, lbdas]} of the fixture, after checking that the generator still makes its problems"""
    if _GOLDEN:
        return _GOLDEN
    spec = importlib.util.spec_from_file_location("make_init_golden",
                                                  os.path.join(HERE, "golden", "make_init_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from oracle import dense_kkt
    d = np.load(GOLDEN)
    probs = golden_problems()
    assert str(d["inputs_sha256"]) == gen.inputs_sha256(probs.values()), "the generator changed: regenerate the fixture"
    assert float(d["mueq"]) == GOLDEN_MUEQ
    for name, prob in probs.items():
        _GOLDEN[name] = list(dense_kkt.dense_solution_to_traj(prob, d[name]))
    return _GOLDEN


# family -> (GAR_HIP_* switches, legs, dense, {set: kernel}).  The kernel names are the ones the row is about: the leg
# family runs the unconstrained sets (the constrained one in leg mode is another family, rows L3 / L4); two legs need
# four knots at least, which the padded set (N = 3) has, each leg two.
GOLDEN_FAMILIES = {
    "wave": ({"BACKWARD": "wave"}, 1, False, {"plain": "wave<8,4>", "padded": "wave<8,4>", "cstr": "wave<8,4,4>"}),
    "wg4": ({"BACKWARD": "wg4"}, 1, False, {"plain": "mfma<8,4>", "padded": "mfma<8,4>"}),
    "leg2": ({}, 2, False, {"plain": "wave_leg<8,4>", "padded": "wave_leg<8,4>"}),
    "dense": ({}, 1, True, {"plain": "dense", "padded": "dense", "cstr": "dense"}),
}


def golden_cases():
    return [(fam, g, kind) for fam, v in GOLDEN_FAMILIES.items() for g, kind in golden_keys() if g in v[3]]


def family_oracle(family, prob):
    """The CPU oracle of the family's algorithm on `prob`: the Riccati oracle serial in time, its leg-parallel solver,
    the stage-dense oracle (oracle/dense_riccati.py) -- what check_serial, check_parallel and check_dense compare with."""
    _, legs, dense, _ = GOLDEN_FAMILIES[family]
    sol = lqrInitializeSolution(prob)
    if dense:
        o = pc.OracleDense(prob)
        o.backward(GOLDEN_MUEQ)
        o.forward(*sol)
    elif legs > 1:
        o = pc.ora.ParallelRiccatiSolver(pc.to_oracle(prob), legs)
        assert o.backward(GOLDEN_MUEQ)
        o.forward(*sol)
    else:
        _, _, sol = pc.oracle_serial(prob, GOLDEN_MUEQ)
    return sol


_GOLDEN_BAR = {}


def golden_bar(family, gset, kind):
    """per part: max(1e-11, CONDITIONING_MARGIN x e_ref), e_ref the error of the family's CPU oracle against the exact
    solution -- measured on the CPU, never on the library.  -> (bar, that oracle's solution, e_ref)"""
    _, legs, dense, _ = GOLDEN_FAMILIES[family]
    key = (dense, legs, gset, kind)
    if key not in _GOLDEN_BAR:
        ref = family_oracle(family, golden_problem(gset, kind))
        e_ref = pc.golden_errors(ref, load_golden()[f"{gset}_{kind}"])
        _GOLDEN_BAR[key] = ([max(GOLDEN_FLOOR, pc.CONDITIONING_MARGIN * e) for e in e_ref], ref, e_ref)
    return _GOLDEN_BAR[key]


def check_golden_case(family, gset, kind, lib_path=None):
    """X1 -> (error against the oracle, error against the exact solution), both relative"""
    from aligator_amd.gar import ParallelRiccatiSolver, ProximalRiccatiSolver, RiccatiSolverDense
    opts, legs, dense, kernels = GOLDEN_FAMILIES[family]
    prob = golden_problem(gset, kind)
    premises(("X1", gset, kind), prob, kind, GOLDEN_MUEQ)
    bar, ref, _ = golden_bar(family, gset, kind)
    exact = load_golden()[f"{gset}_{kind}"]
    with sf.options(INIT=None, **opts):
        if dense:
            s = RiccatiSolverDense(prob, lib_path=lib_path)
        elif legs > 1:
            s = ParallelRiccatiSolver(prob.copy(), legs, lib_path=lib_path)
        else:
            s = ProximalRiccatiSolver(prob, lib_path=lib_path)
    assert s.kernel_name == kernels[gset], (s.kernel_name, kernels[gset])
    assert s.backward(GOLDEN_MUEQ)
    sol = lqrInitializeSolution(prob)
    assert s.forward(*sol)
    assert s._impl.num_failed() == 0
    errs = pc.golden_errors(sol, exact)
    oerr = rel_error(sol, ref)
    print(f"init-report X1_{family}_{gset} {kind} oracle {oerr:.2e} exact {max(errs):.2e}")
    for part, (e, b) in enumerate(zip(errs, bar)):
        assert e <= b, (family, gset, kind, part, errs, bar)
    assert_kkt(prob, sol, ref, GOLDEN_MUEQ, 1e-9)
    return oerr, max(errs)
