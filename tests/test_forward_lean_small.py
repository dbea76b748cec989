"""gar_forward_lean (csrc/gar_forward_lean.hpp) at its smallest sizes: the roll-out of the pipelined schedule must be
bit for bit the one of gar_forward_mfma where its stage pipeline is still filling -- N = 1, 2, 3: the prologue only,
the first refill of the two LDS buffers, the first steady-state stage -- and where its four-wave workgroup is not full.

Every case runs the lean roll-out twice over: in the pipelined schedule (where the library offers it: two problems or
more; the halves of a batch of 4 / 5 hold 2 + 2 / 3 + 2 problems) and, for the WHOLE batch in one launch, in the plain
schedule under GAR_HIP_FORWARD=lean -- one wave, one full workgroup of four waves, a partial second workgroup.  Both
against the plain schedule with its default roll-out, all solutions compared with ==.  Each run is two steps back to
back with no synchronisation between them: the DMA pieces in flight of consecutive stages and launches, and anything a
wave keeps in its LDS slice from one stage to the next, would show an overlap.  The last test puts a general initial
stage into both halves: the roll-out of a half must see the x0 that gar_initial_wave writes behind that half's sweep,
whatever else the schedule lets run in between.

CPU: the unmodified sources on the lane-per-thread emulator.  GPU (-m gpu): the real library."""
import os
import subprocess

import numpy as np
import pytest

from aligator_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "_build", "libgar_hip_emu.so")

SHAPES = [(36, 12), (32, 12), (12, 4)]
HORIZONS = [1, 2, 3]
BATCHES = [1, 4, 5]
CASES = [(nx, nu, N, batch) for nx, nu in SHAPES for N in HORIZONS for batch in BATCHES]


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu")], check=True)
    return EMU


def _solutions(s):
    s.sync()
    assert s.num_failed() == 0
    return [[[a.copy() for a in part] for part in s.solution(b)] for b in range(s.batch)]


def _steps(s, mu, steps=2):
    for _ in range(steps):
        s.backward_async(mu)
        s.forward_async()
    return _solutions(s)


def _assert_same_bits(ref, got, what):
    for b, (P, Q) in enumerate(zip(ref, got)):
        for X, Y in zip(P, Q):
            for x, y in zip(X, Y):
                assert np.array_equal(x, y), (what, b)


def _solver(lib, probs, monkeypatch):
    from aligator_amd.gar import BatchedRiccatiSolver
    monkeypatch.setenv("GAR_HIP_BACKWARD", "wave")        # the one-wave-per-problem family at any batch size
    nx, nu = probs[0].stages[0].dims[0], probs[0].stages[0].dims[1]
    s = BatchedRiccatiSolver([k.dims for k in probs[0].stages], nx, batch=len(probs), lib_path=lib)
    assert s.kernel_name == f"wave<{nx},{nu}>"
    s.upload(probs)
    return s


def _check(lib, nx, nu, N, batch, monkeypatch):
    probs = [synth.generate_lq_problem(900 + i, np.linspace(-1, 1, nx) * (i + 1), N, nx, nu, mode="W")
             for i in range(batch)]
    s = _solver(lib, probs, monkeypatch)
    s.set_pipeline(0)
    plain = _steps(s, 1e-12, steps=1)
    assert max(float(np.abs(x).max()) for P in plain for X in P for x in X if x.size) > 0
    monkeypatch.setenv("GAR_HIP_FORWARD", "lean")         # (read per launch) the whole batch in one lean launch
    _assert_same_bits(plain, _steps(s, 1e-12), "lean roll-out, plain schedule")
    monkeypatch.delenv("GAR_HIP_FORWARD")
    if batch >= 2:                                        # (the pipelined schedule is not offered to a single problem)
        s.set_pipeline(2)
        assert s.pipeline == 2
        _assert_same_bits(plain, _steps(s, 1e-12), "pipelined schedule")
        s.set_pipeline(0)
        _assert_same_bits(plain, _steps(s, 1e-12, steps=1), "plain schedule behind the pipelined one")
    s.close()


def _check_general_initial_stage(lib, nx, nu, N, batch, monkeypatch):
    """G0 is not +-I in problems of BOTH halves (problem 0 keeps -I): the sweep flags them and gar_initial_wave, launched
    behind the sweep, writes the x0 that the roll-out of that half starts from.  The reference is the plain schedule
    (the same factorisation of [Vxx0 G0^T; G0 0], fused into its sweep).  Two pipelined steps with no sync between."""
    rng = np.random.default_rng(11)
    probs = [synth.generate_lq_problem(950 + i, np.zeros(nx), N, nx, nu, mode="W") for i in range(batch)]
    for p in probs[1:]:
        p.G0[...] = -np.eye(nx) + 0.3 * rng.standard_normal((nx, nx))
        p.g0[...] = rng.standard_normal(nx)
    s = _solver(lib, probs, monkeypatch)
    s.set_pipeline(0)
    plain = _steps(s, 1e-12, steps=1)
    s.set_pipeline(2)
    piped = _steps(s, 1e-12)
    first = (batch + 1) // 2
    assert first >= 2 and batch - first >= 1              # perturbed problems in both halves
    _assert_same_bits(plain, piped, "pipelined schedule, general initial stage")
    from aligator_amd.gar import lqrComputeKktError
    for b, p in enumerate(probs):                         # ... and the solution is one: not two copies of a mistake
        scale = max(1.0, max(float(np.abs(v).max()) for part in piped[b] for v in part if v.size))
        assert max(lqrComputeKktError(p, *piped[b], mueq=1e-12)) <= 1e-9 * scale
    s.close()


@pytest.mark.parametrize("nx,nu,N,batch", CASES)
def test_lean_roll_out_is_bitwise_the_default_roll_out(emu, monkeypatch, nx, nu, N, batch):
    _check(emu, nx, nu, N, batch, monkeypatch)


def test_lean_roll_out_sees_the_deferred_initial_stage(emu, monkeypatch):
    _check_general_initial_stage(emu, 12, 4, 3, 5, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("nx,nu,N,batch", CASES)
def test_gpu_lean_roll_out_is_bitwise_the_default_roll_out(monkeypatch, nx, nu, N, batch):
    _check(None, nx, nu, N, batch, monkeypatch)


@pytest.mark.gpu
def test_gpu_lean_roll_out_sees_the_deferred_initial_stage(monkeypatch):
    _check_general_initial_stage(None, 36, 12, 3, 5, monkeypatch)
