"""Gradients of a resident batch (gar_hip_adjoint, gar_hip_adjoint_async, gar_hip_upload_packed_user_device,
gar_hip_solution_vectors_device, aligator_amd/layer.py) on the emulator: tests/adjoint_cases.py's checks on the CPU build
of the unmodified kernel sources (tests/emu) -- the five kernels of gar_adjoint.hpp (stage descriptors, ring slots, packed
triangles, the fbT2 order, padding), the redirected sweep and initial stage they share with the refinement, the host side
of the entry points and the PyTorch layer on CPU tensors.  GPU execution is tests/test_adjoint_gpu.py's.

Largest ratios seen on the emulator: adjoint over the library's full solve of the substituted problem (margin 10) 4.23;
gradient entries over their bound 4 eps (|ab| + |cd|) 0.000 (the host has no FMA: numpy rounds as the emulated kernel does); gradient against autograd over its bar 0.001."""
import ctypes as C
import os
import subprocess

import pytest

import adjoint_cases as adc

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "emu", "_build", "libgar_hip_emu.so")


@pytest.fixture(scope="module", autouse=True)
def build_emu():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu")], check=True)


SERIAL = [(8, 4, 5, 3, "wave<8,4>", dict(BACKWARD="wave")), (8, 4, 5, 3, "mfma<8,4>", dict(BACKWARD="wg4")),
          (8, 4, 5, 3, "generic", dict(FORCE_GENERIC="1")), (36, 12, 4, 2, "wave<36,12>", dict(BACKWARD="wave")),
          (5, 3, 3, 3, "generic", dict(FORCE_GENERIC="1"))]


@pytest.mark.parametrize("nx,nu,N,batch,kernel,opts", SERIAL, ids=[f"{r[4]}-{r[0]}" for r in SERIAL])
def test_serial_families(nx, nu, N, batch, kernel, opts):
    adc.check_serial(LIB, nx, nu, N, batch, kernel, **opts)


@pytest.mark.parametrize("nx,nu,N,kernel", [(4, 2, 6, "wave<8,4>"), (12, 6, 6, "wave<12,8>"), (56, 22, 3, "pair<56,24>")])
def test_padded_solvers_in_the_callers_dimensions(nx, nu, N, kernel):
    adc.check_padded(LIB, nx, nu, N, kernel)


INITIAL = [(0, "-I")] + [(f, k) for f in (1, 2) for k in adc.isc.G0_KINDS]


@pytest.mark.parametrize("init", [None, "bk"], ids=["default", "bk"])
@pytest.mark.parametrize("frac,kind", INITIAL, ids=[f"nc0={('0', 'nx/2', 'nx')[f]},G0={k}" for f, k in INITIAL])
def test_initial_stage(frac, kind, init):
    adc.check_initial(LIB, frac, kind, init)


@pytest.mark.parametrize("which", ["nx2=0", "one knot", "nu>0"])
def test_terminal_knot_edge_cases(which):
    adc.check_terminal(LIB, which)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_ring_after_two_cycle_appends(family):
    adc.check_ring(LIB, family)


def test_grid_indexing_over_seventy_problems():
    adc.check_grid(LIB)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_what_must_not_move(family):
    adc.check_untouched(LIB, family)


def test_failed_problem_gets_zero_records():
    adc.check_failed_problem(LIB)


@pytest.mark.parametrize("what", ["nc", "nth", "legs", "dense", "no backward", "no forward", "null cotangent"])
def test_refusals_leave_everything_alone(what):
    adc.check_refusals(LIB, what)


def test_multi_device_handle_is_refused():
    lib = C.CDLL(LIB)
    lib.emu_set_device_count(2)      # two virtual devices
    try:
        adc.check_refusals(LIB, "multi", devices=(0, 1))
    finally:
        lib.emu_set_device_count(1)


def test_allocation_counts():
    adc.check_allocation(LIB, rounds=20)


@pytest.mark.parametrize("pipeline", [False, True], ids=["plain", "pipelined"])
def test_no_host_synchronisation(pipeline):
    adc.check_no_host_sync(LIB, pipeline=pipeline)


def test_new_matrices_invalidate_until_the_next_backward():
    adc.check_invalidation(LIB)


@pytest.mark.parametrize("kind", ["plain", "qr-packed", "padded"])
def test_device_round_trip_of_the_callers_packed_problems(kind):
    adc.check_round_trip(LIB, kind)


def test_layer_on_cpu_tensors():
    adc.check_layer(LIB, "cpu")
