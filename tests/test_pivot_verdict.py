"""The plain stage's register LDL^T gives ONE pivot verdict per factorisation in its default mode (gar_wave2.hpp:
wave_ldl_fast_neg_spd): the column loop only collects the lanes that fail the first Bunch-Kaufman test and the sign
of the pivots, and what used to be decided column by column is decided behind the last column; under
GAR_HIP_SPD_ACCEPT=0 the per-column routine runs as before.  One batch of four problems on `wave<36,12>`, N = 4,
walks every outcome in both modes; every wave sweeps common stages and one special stage:

  0  every column of every stage passes the first test;
  1  a column fails the first test and Rhat is positive definite: accepted unpivoted by default; under
     GAR_HIP_SPD_ACCEPT=0 the second test runs and either keeps kp = k ("keeps") or makes Bunch-Kaufman interchange
     ("interchanges": positive pivots throughout, so only the literal rule leaves the register factorisation);
  2  Rhat is indefinite: Bunch-Kaufman takes 2x2 pivots, the stage runs the device Bunch-Kaufman;
  3  Rhat = 0: an exactly zero pivot column, the problem's status word is set.

The premises are checked on the oracle (its Rhat, its pivot sequence) before anything is compared; the counters
expected of the library are derived from the oracle's Rhat, not from the library.  Factors and solutions at the
1e-9 that parity_cases.check_second_bunch_kaufman_test holds these families to (generator "W")."""
import os

import numpy as np
import pytest

from aligator_amd import synth
from aligator_amd.gar import BatchedRiccatiSolver
from oracle import oracle as ora
import parity_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "_build", "libgar_hip_emu.so")
LIBS = [pytest.param(EMU, id="emu"), pytest.param(None, id="gpu", marks=pytest.mark.gpu)]

NX, NU, N, MU = 36, 12, 4, 1e-12
ALPHA = (1.0 + np.sqrt(17.0)) / 8.0
# the 4 x 4 heads of parity_cases.check_second_bunch_kaufman_test
KEEP = np.array([[1.0, 2.0, 0.0, 0.0], [2.0, 10.0, 3.0, 0.0], [0.0, 3.0, 20.0, 0.1], [0.0, 0.0, 0.1, 4.0]])
PIVOT = KEEP.copy()
PIVOT[2, 1] = PIVOT[1, 2] = 0.5
TWO = np.array([[0.1, 5.0, 0.0, 0.0], [5.0, 0.2, 1.0, 0.0], [0.0, 1.0, 20.0, 0.1], [0.0, 0.0, 0.1, 4.0]])


def embed(head):
    """head in the leading block of an NU x NU matrix whose other columns pass the first test"""
    M = np.diag(np.linspace(3.0, 9.0, NU))
    M[np.arange(4, NU - 1), np.arange(5, NU)] = M[np.arange(5, NU), np.arange(4, NU - 1)] = 0.25
    M[:4, :4] = head
    return M


def special(prob, t, Rm):
    k = prob.stages[t]
    k.R[...] = Rm
    k.S[...] = 0.0
    k.B[...] = 0.0                                           # Rhat = R at this stage


def unpivoted(Rhat):
    """(some column fails the first test, every pivot is positive) of the unpivoted elimination the kernel runs"""
    a = np.array(Rhat, dtype=float)
    fails, positive = False, True
    for k in range(a.shape[0]):
        col = np.abs(a[k:, k])
        fails |= bool((~(abs(a[k, k]) >= ALPHA * col)).any() or a[k, k] == 0.0)
        positive &= bool(a[k, k] > 0.0)
        if a[k, k] == 0.0:
            return True, False
        a[k + 1:, k + 1:] -= np.outer(a[k + 1:, k], a[k + 1:, k]) / a[k, k]
    return fails, positive


def build(second_test):
    probs = [synth.generate_lq_problem(31 + b, np.zeros(NX), N, NX, NU, mode="W") for b in range(4)]
    special(probs[1], 1, embed(KEEP if second_test == "keeps" else PIVOT))
    special(probs[2], 1, embed(TWO))
    special(probs[3], 0, np.zeros((NU, NU)))                 # (the last stage swept: nothing runs on its NaNs)
    return probs


def expected_counters(probs, spd):
    """(stages that fail the first test, those of them that leave the register factorisation), from the oracle"""
    first = left = 0
    osols = []
    for b, p in enumerate(probs[:3]):
        _, osol, ref = pc.oracle_serial(p, MU)
        osols.append((osol, ref))
        for t in range(N):
            Rhat = osol.datas(t).Rhat
            fails, positive = unpivoted(Rhat)
            keeps = np.array_equal(ora.BunchKaufman(Rhat).pivots, np.arange(NU))
            first += fails
            left += fails and (not positive if spd else not keeps)
            if not fails:
                assert keeps, (b, t)
    assert not pc.reference_solvable(probs[3], MU)
    # problem 3: its stages N-1 .. 1 are those of the same problem without the special stage; at stage 0 the zero
    # column fails the first test and the stage is refused
    _, osol, _ = pc.oracle_serial(synth.generate_lq_problem(31 + 3, np.zeros(NX), N, NX, NU, mode="W"), MU)
    for t in range(1, N):
        fails, _ = unpivoted(osol.datas(t).Rhat)
        assert not fails, t
    return (first + 1, left + 1), osols


def test_premises_land_in_their_branches():
    for second_test in ("keeps", "interchanges"):
        probs = build(second_test)
        per = []
        for p in probs[:3]:
            _, osol, _ = pc.oracle_serial(p, MU)
            rows = []
            for t in range(N):
                Rhat = osol.datas(t).Rhat
                fails, positive = unpivoted(Rhat)
                rows.append((fails, positive, np.array_equal(ora.BunchKaufman(Rhat).pivots, np.arange(NU)),
                             int((ora.BunchKaufman(Rhat).pivots < 0).sum())))
            per.append(rows)
        assert all(r == (False, True, True, 0) for r in per[0])                               # case 0
        assert [r[0] for r in per[1]] == [False, True, False, False]                          # case 1: stage 1 only
        assert per[1][1][1] and per[1][1][2] == (second_test == "keeps")
        assert np.linalg.eigvalsh(probs[1].stages[1].R).min() > 0
        assert [r[0] for r in per[2]] == [False, True, False, False]                          # case 2
        assert not per[2][1][1] and not per[2][1][2] and per[2][1][3] == 2
        assert np.linalg.eigvalsh(probs[2].stages[1].R).min() < 0
        assert expected_counters(probs, True)[0] == (3, 2)
        assert expected_counters(probs, False)[0] == ((3, 2) if second_test == "keeps" else (3, 3))


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("spd", ["1", "0"])
@pytest.mark.parametrize("second_test", ["keeps", "interchanges"])
def test_one_verdict_per_factorisation(monkeypatch, lib, spd, second_test):
    monkeypatch.setenv("GAR_HIP_BACKWARD", "wave")
    monkeypatch.setenv("GAR_HIP_SPD_ACCEPT", spd)
    probs = build(second_test)
    want, osols = expected_counters(probs, spd == "1")
    s = BatchedRiccatiSolver([k.dims for k in probs[0].stages], probs[0].nc0, batch=4, lib_path=lib)
    assert s.kernel_name == f"wave<{NX},{NU}>"
    s.upload(probs)
    pc.assert_reported_failure(s.backward, MU)
    st = s.status()
    assert [bool(v) for v in st] == [False, False, False, True], st
    assert s.num_failed() == 1
    assert s.slow_path_stages() == want
    s.forward()
    for b, (osol, ref) in enumerate(osols):
        for A, B in zip(s.solution(b), ref):
            assert pc.maxdiff(A, B) <= 1e-9 * pc.scale_of(ref), b

        class D:
            def __getitem__(self, t, b=b):
                return s.factor(t, b)
        pc.compare_factors(D(), osol, N, 1e-9, names=("ff", "fb"), vnames=("Vxx", "vx"))


@pytest.mark.parametrize("lib", LIBS)
def test_terminal_and_initial_stage_alone(monkeypatch, lib):
    monkeypatch.setenv("GAR_HIP_BACKWARD", "wave")
    prob = synth.generate_lq_problem(5, np.ones(NX), 1, NX, NU, mode="W")
    solver, _, _ = pc.check_serial(prob, MU, 1e-9, lib, kkt_tol=1e-9)
    assert solver.kernel_name == f"wave<{NX},{NU}>"
    assert solver._impl.slow_path_stages() == (0, 0)
