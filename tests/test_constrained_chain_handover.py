"""The serial constrained family `wave<NX,NU,NC>` sweeps a problem with a chain of three kernels on one stream
(gar_wave.hpp: gar_backward_wave_body, PHASE 0 / 1 / 2): a kernel that meets a knot it does not serve writes the knot
into MfmaParams::resume[b] and leaves, the next one rebuilds V', vx' from the record of knot t+1 and carries on.  One
batch per shape (chain_handover_cases.SCRIPTS, N = 6) hands over at N-1, at N-2, in the interior, at 1 and at 0, once and
twice, out of either kernel, with the closed-form and the Bunch-Kaufman initial stage in each of the three kernels, next
to a problem that fails -- every problem of the batch on a path of its own, so that resume[b], status[b] and the early
exits are indexed with b > 0.

The premises are checked on the oracle alone (test_premises_land_in_their_kernels); the stage counters expected of the
library come from the oracle-derived map.  Each (shape, library) case, twice on one solver -- the second time with the
problems rotated by 5 slots, so that every slot finishes in another kernel and nothing of resume, the status words or
the counters may survive a sweep:
  1  kernel name, reported failure, status() flags the failing problem alone, num_failed() == 1;
  2  constrained_bk_stages() == the (coupled, Bunch-Kaufman) totals of the map;
  3  every other problem against the oracle: ff, fb, Vxx, vx of every stage, kkt0, the solution at 1e-8 relative
     (`conditioned` as parity_cases.check_serial applies it), lqrComputeKktError at check_serial's bound;
  4  ... and bitwise equal to the same problem alone on a batch-1 solver of the family (same kernels, same path, no
     arithmetic across problems: a difference is an indexing error).

The emulator (one OS thread per lane) runs the full batch at every shape: (36, 12, 32) takes 75 ... 100 s there, (16, 8, 8)
15 ... 20 s, (8, 4, 4) 11 ... 14 s; on the GPU a case is well under two seconds."""
import os
import subprocess

import numpy as np
import pytest

from aligator_amd.gar import BatchedRiccatiSolver
import chain_handover_cases as ch
import parity_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "_build", "libgar_hip_emu.so")
LIBS = [pytest.param(EMU, id="emu"), pytest.param(None, id="gpu", marks=pytest.mark.gpu)]


def rotated(names):
    return tuple(names[(i + ch.ROTATE) % len(names)] for i in range(len(names)))


def test_premises_land_in_their_kernels():
    assert sorted(ch.ORDER) == sorted(ch.SCRIPTS)
    # the rotation changes the kernel every slot finishes in
    assert all(ch.finishing_kernel(a) != ch.finishing_kernel(b) for a, b in zip(ch.ORDER, rotated(ch.ORDER)))
    assert {ch.finishing_kernel(n) for n in ch.ORDER} == {0, 1, 2}
    # the scripts, from the oracle's Rhat and pivot sequences alone (chain_handover_cases.premise: the kernel of every
    # knot is the table's, every common and every designated coupled knot passes the first Bunch-Kaufman test in
    # every column of the unpivoted elimination, every knot forced to pivot takes 2x2 pivots)
    for shape in ch.SHAPES:
        for name in ch.SCRIPTS:
            assert ch.premise(shape, name) is None, (shape, name, ch.premise(shape, name))
            prob = ch.reference(shape, name)[0]
            assert pc.reference_solvable(prob, ch.MU[shape]) == (name != ch.FAILING), (shape, name)
        nx, nu, nc = shape
        for name, (i, j) in (("J", (nc - 1, nu - 1)), ("J2", (0, nu - 1))):   # one entry of D, in the last column
            D = ch.reference(shape, name)[0].stages[3].D
            assert D[i, j] == 0.5 and np.count_nonzero(D) == 1
        for name in ("A'", "E'", "I'"):                  # no closed form for the initial stage
            G0 = ch.reference(shape, name)[0].G0
            assert np.count_nonzero(G0 - np.diag(np.diag(G0))) > 0
    # the table of the issue, as totals: 16 problems x 6 knots
    assert ch.expected_stages(ch.ORDER) == (28, 17)
    assert ch.expected_stages(("F",)) == (0, 3) and ch.expected_stages(("G",)) == (3, 2)
    assert ch.expected_stages((ch.FAILING,)) == (0, ch.T_FAIL + 1)


def solve_alone(shape, lib):
    """name -> Result of the problem alone on ONE batch-1 solver of the family, reused from problem to problem"""
    nx, nu, nc = shape
    p0 = ch.reference(shape, "A")[0]
    s = BatchedRiccatiSolver([k.dims for k in p0.stages], p0.nc0, batch=1, lib_path=lib)
    assert s.kernel_name == f"wave<{nx},{nu},{nc}>"
    out = {}
    for name in ch.SCRIPTS:
        if name == ch.FAILING:
            continue
        s.upload([ch.reference(shape, name)[0]])
        assert s.backward(ch.MU[shape]) and s.forward()
        assert s.constrained_bk_stages() == ch.expected_stages((name,)), name
        out[name] = ch.Result(s, 0)
    return out


def check_sweep(s, alone, shape, names):
    mu = ch.MU[shape]
    s.upload([ch.reference(shape, n)[0] for n in names])
    pc.assert_reported_failure(s.backward, mu)                                               # 1
    st = s.status()
    assert [bool(v) for v in st] == [n == ch.FAILING for n in names], st
    assert s.num_failed() == 1
    assert s.constrained_bk_stages() == ch.expected_stages(names)                            # 2
    s.forward()
    for b, name in enumerate(names):
        if name == ch.FAILING:
            continue
        res = ch.Result(s, b)
        ch.compare_with_oracle(res, shape, name)                                             # 3
        for i, (x, y) in enumerate(zip(res.arrays(), alone[name].arrays())):                 # 4
            assert np.array_equal(x, y), (name, b, i, float(np.abs(x - y).max()))


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("shape", ch.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_handover_at_every_knot_across_a_batch(shape, lib):
    if lib == EMU:
        subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu")], check=True)
    nx, nu, nc = shape
    names = ch.ORDER
    p0 = ch.reference(shape, names[0])[0]
    s = BatchedRiccatiSolver([k.dims for k in p0.stages], p0.nc0, batch=len(names), lib_path=lib)
    assert s.kernel_name == f"wave<{nx},{nu},{nc}>"
    alone = solve_alone(shape, lib)
    check_sweep(s, alone, shape, names)
    check_sweep(s, alone, shape, rotated(names))
