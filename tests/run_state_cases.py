"""What a caller reads back while the solver's cached results are in play (the factor records, the side
buffer W, the solution in HBM, the pinned host copies of the solution and of the gains): cases and checks shared by the
emulator tests (tests/test_run_state.py) and the GPU tests (tests/test_run_state_gpu.py).

The judge is a second solver B of the same family that performs the same mathematical sequence with no cache in play:
upload + backward + forward in place of backward_blocks, and no prefetch_gains call.  The kernels and their inputs are
the same on both, so every fetch_results buffer (solution, ff_all, fb_all) of A must EQUAL B's, bit for bit -- there is
no tolerance.  The emulator executes streams synchronously, so it checks the state rules; on the GPU the same cases also
check the ordering of the asynchronous copies on the second stream.

A scenario is a list of steps, written once and played on both solvers (play): B expands or drops the cached ones."""
import numpy as np
import pytest

from aligator_amd import synth
import affine_cases as ac
import kkt_device_cases as kc
import parity_cases as pc

MUEQ = 1e-8


def fetched(s, b, solution, gains):
    """copies of what fetch_results hands out (views of the library's pinned buffer, valid until the next fetch)"""
    return [None if a is None else a.copy() for a in s.fetch_results(b, solution=solution, gains=gains)]


def play(s, steps, cached):
    """-> the fetched buffers, in order.  cached = False: the judge's form of the same sequence"""
    out = []
    for op, *a in steps:
        if op == "blocks" and cached:
            assert s.backward_blocks(a[0][0], MUEQ)
        elif op == "blocks":
            s.upload(a[0])
            assert s.backward(MUEQ) and s.forward()
        elif op == "blocks fails" and cached:
            pc.assert_reported_failure(lambda m: s.backward_blocks(a[0][0], m), MUEQ)
        elif op == "blocks fails":
            s.upload(a[0])
            pc.assert_reported_failure(s.backward, MUEQ)
        elif op == "upload":
            s.upload(a[0])
        elif op == "backward":
            assert s.backward(MUEQ)
        elif op == "forward":
            assert s.forward()
        elif op == "prefetch":
            if cached:
                s.prefetch_gains(a[0])
        elif op == "collapse":
            s.collapse_feedback()
        elif op == "affine":
            s.upload_affine(ac.affine_of(s, a[0]))
            assert s.backward_affine()
        elif op == "cycle":                 # a ring turn, then the new last-but-one knot
            s.cycle_append(a[0].dims)
            s.upload_knot(0, s.horizon - 1, a[0])
        elif op == "fetch":
            out.append(fetched(s, *a))
        else:
            raise AssertionError(op)
    return out


def failing(prob):
    """affine_cases.check_failed_problem's recipe: R-hat = 0 at one knot"""
    p = prob.copy()
    bad = p.stages[2]
    bad.R[...] = 0.0
    bad.S[...] = 0.0
    bad.B[...] = 0.0
    return p


def scenario(n, P, Q):
    """A's steps of scenario n; P, Q: two batches of problems of the solver's dimensions"""
    both = ("fetch", 0, True, True)
    if n == 1:
        return [("blocks", P), ("forward",), both]
    if n == 2:
        return [("blocks", P), both]
    if n == 3:
        return [("blocks", P), ("prefetch", 0), ("forward",), both]
    if n == 4:
        return [("upload", P), ("backward",), ("prefetch", 0), ("forward",), both]
    if n == 5:
        return [("upload", P), ("backward",), ("prefetch", 0), ("upload", Q), ("backward",), ("forward",), both]
    if n == 6:
        return [("upload", P), ("backward",), ("prefetch", 1), ("fetch", 0, False, True)]
    if n == 7:
        return [("blocks", P), ("collapse",), ("forward",), both]
    if n == 8:
        return [("upload", P), ("backward",), ("prefetch", 0), ("collapse",), ("fetch", 0, False, True)]
    if n == 9:
        sub = [ac.substituted(p, np.random.default_rng(61)) for p in P]
        return [("blocks", P), ("forward",), ("affine", sub), ("forward",), ("fetch", 0, True, False)]
    if n == 10:
        k = P[0].stages[0]
        knot = synth.generate_knot(np.random.default_rng(67), k.nx, k.nu, mode="W")
        return [("blocks", P), ("cycle", knot), ("backward",), ("forward",), both]
    if n == 11:
        return [("blocks fails", [failing(P[0])]), ("blocks", P), ("forward",), both]
    raise AssertionError(n)


# scenario -> (nx, nu, N, batch, legs)
SERIAL, LEGS = (8, 4, 5, 1, 1), (8, 4, 11, 1, 3)
SHAPES = {n: SERIAL for n in (1, 2, 3, 4, 5, 9, 10, 11)}
SHAPES.update({6: (8, 4, 5, 2, 1), 7: LEGS, 8: LEGS})
CASES = [(n, SHAPES[n]) for n in sorted(SHAPES)] + [(1, (4, 2, 5, 1, 1))]        # (the last: padded onto wave<8,4>)
IDS = [f"scenario{n}-nx{sh[0]}-N{sh[2]}-batch{sh[3]}-legs{sh[4]}" for n, sh in CASES]


def check_scenario(lib_path, n, shape):
    nx, nu, N, batch, legs = shape
    P, Q = kc.unconstrained(nx, nu, N, batch, seed=20 + n), kc.unconstrained(nx, nu, N, batch, seed=40 + n)
    A = kc.solver_for(P, lib_path, num_legs=legs, BACKWARD="wave")
    B = kc.solver_for(P, lib_path, num_legs=legs, BACKWARD="wave")
    if legs == 1:
        assert A.kernel_name == "wave<8,4>" and A.padded == (nx != 8), (A.kernel_name, A.padded)
    assert A.kernel_name == B.kernel_name
    steps = scenario(n, P, Q)
    got, want = play(A, steps, cached=True), play(B, steps, cached=False)
    assert len(got) == len(want) >= 1
    for g, w in zip(got, want):
        for name, x, y in zip(("solution", "ff_all", "fb_all"), g, w):
            assert (x is None) == (y is None), name
            if x is not None:
                assert x.size and np.isfinite(y).all() and np.abs(y).max() > 0, name      # (the judge holds a result)
                assert np.array_equal(x, y), (n, name, int((x != y).sum()))
    if n == 5:      # the second problem's, not the first's: the judge's own fetch of P differs
        first = play(B, [("upload", P), ("backward",), ("forward",), ("fetch", 0, True, True)], cached=False)[0]
        assert not np.array_equal(first[0], got[0][0]) and not np.array_equal(first[2], got[0][2])
    A.close()
    B.close()


# ---- the refusal texts of backward_affine and refine ------------------------------------------------------------------
def check_refusal_texts(lib_path):
    """every refusal of "no factorisation to re-solve / refine from", for both callers: before any backward, after
    each of the five entry points that change matrix blocks (named in the text), and refine's "no forward"."""
    nx, nu, N = 8, 4, 4
    probs, others = kc.unconstrained(nx, nu, N, 2, seed=15), kc.unconstrained(nx, nu, N, 2, seed=16)
    s = kc.solver_for(probs, lib_path, BACKWARD="wg4")
    assert not s.qr_packed and not s.padded           # (upload_packed takes the records as they are: its own site)
    callers = (("gar_hip_backward_affine", "re-solve", s.backward_affine), ("gar_hip_backward_affine", "re-solve", s.backward_affine_async),
               ("gar_hip_refine", "refine", lambda: s.refine(1)), ("gar_hip_refine_async", "refine", lambda: s.refine_async(1)))
    for who, verb, call in callers:
        with pytest.raises(RuntimeError, match=f"gar_hip error -1: {who}: no backward of this solver to {verb} from$"):
            call()
    assert s.backward(MUEQ)
    for who, verb, call in callers[2:]:
        with pytest.raises(RuntimeError, match=f"gar_hip error -1: {who}: no forward since the last backward"):
            call()
    keep_p, packed_dev = ac.to_device(np.concatenate([s.pack_device(p) for p in others]), lib_path)
    keep_d, deriv_dev = ac.to_device(np.zeros(s.batch * s.deriv_doubles), lib_path)
    mutators = (("gar_hip_upload_packed", lambda: s.upload(others)),
                ("gar_hip_upload_packed_device", lambda: s.upload_packed_device(packed_dev)),
                ("gar_hip_upload_stage", lambda: s.upload_knot(0, 1, others[0].stages[1])),
                ("gar_hip_update_lq_subproblem_device", lambda: s.update_lq_subproblem_device(deriv_dev, 1e-6, True)),
                ("gar_hip_cycle_append", lambda: s.cycle_append(probs[0].stages[0].dims)))
    for name, mutate in mutators:
        s.upload(probs)
        assert s.backward(MUEQ) and s.forward()
        assert s.backward_affine() and s.forward() and s.refine(1)[0] == 1            # (served before the change)
        mutate()
        for who, _, call in callers:
            with pytest.raises(RuntimeError, match=f"gar_hip error -1: {who}: matrix blocks changed since the last "
                                                   f"backward \\({name}\\): call gar_hip_backward first$"):
                call()
    s.sync()
    s.close()
