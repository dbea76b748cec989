"""Device-side KKT residuals and per-problem status (gar_hip_kkt_error, gar_hip_get_status) on the emulator:
tests/kkt_device_cases.py's checks on the CPU build of the unmodified kernel sources (tests/emu) -- the index maps of
gar_kkt.hpp (stage descriptors, ring slots, packed triangles, tile ranges, the ownership of the residual entries) and the
host side of the five entry points.  GPU execution is tests/test_kkt_device_gpu.py's."""
import ctypes as C
import os
import subprocess

import pytest

import kkt_device_cases as kc

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "emu", "_build", "libgar_hip_emu.so")


@pytest.fixture(scope="module", autouse=True)
def build_emu():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu")], check=True)

SERIAL = [(8, 4, 5, 3, "wave", "wave<8,4>", True), (8, 4, 5, 3, "wg4", "mfma<8,4>", False),
          (36, 12, 4, 2, "wave", "wave<36,12>", True)]


@pytest.mark.parametrize("nx,nu,N,batch,family,kernel,packed", SERIAL)
def test_serial_families_packed_and_full_records(nx, nu, N, batch, family, kernel, packed):
    kc.check_serial(LIB, nx, nu, N, batch, family, kernel, packed)


@pytest.mark.parametrize("D", [False, True])
def test_headline_constrained_family(D):
    kc.check_constrained_serial(LIB, 36, 12, 32, 3, D, "wave<36,12,32>")


def test_any_dimension_kernels_with_a_random_D():
    kc.check_constrained_serial(LIB, 8, 4, 4, 5, True, "generic", FORCE_GENERIC="1")


@pytest.mark.parametrize("fold", [False, True])
def test_mixed_nc_with_and_without_the_serial_fold(fold):
    kc.check_mixed_nc(LIB, fold)


@pytest.mark.parametrize("nx,nu,N,kernel", [(4, 2, 6, "wave<8,4>"), (12, 6, 6, "wave<12,8>"), (56, 22, 3, "pair<56,24>")])
def test_padded_solvers_in_the_callers_dimensions(nx, nu, N, kernel):
    kc.check_padded(LIB, nx, nu, N, kernel)


@pytest.mark.parametrize("kind", ["plain", "fold", "cstr_seg"])
def test_leg_mode(kind):
    kc.check_legs(LIB, kind)


def test_dense_solver():
    kc.check_dense(LIB)


def test_parameterised_serial_with_theta_and_without():
    kc.check_parameterised(LIB)


def test_terminal_knot_without_next_state():
    kc.check_terminal_nx2_zero(LIB)


def test_one_knot():
    kc.check_one_knot(LIB)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_ring_after_two_cycle_appends(family):
    kc.check_ring(LIB, family)


def test_grid_indexing_over_seventy_problems():
    kc.check_grid(LIB)


def test_pipelined_schedule_without_host_synchronisation():
    kc.check_pipelined(LIB)


def test_failed_problems_are_named_and_show_in_the_residuals():
    kc.check_failures(LIB)


def test_allocation_counts():
    kc.check_allocation(LIB, rounds=20)


def test_multi_device_handle_is_refused():
    lib = C.CDLL(LIB)
    lib.emu_set_device_count(2)      # two virtual devices
    try:
        kc.check_multi_device(LIB, devices=(0, 1))
    finally:
        lib.emu_set_device_count(1)
