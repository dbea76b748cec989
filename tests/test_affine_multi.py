"""A resident batch solved for many affine terms at once (gar_hip_affine_solve_multi, gar_hip_affine_solve_multi_async,
aligator_amd/layer.py: lq_affine_solve_multi) on the emulator: tests/affine_multi_cases.py's checks on the CPU build of the
unmodified kernel sources (tests/emu) -- the four kernels of gar_affine_multi.hpp (the panel scatter, the MFMA sweep and
roll-out with their tile edges, packed triangles, the fbT2 order, padding, ring slots, the per-column initial stage), the
host side of the entry points (chunks, staging, state rules) and the layer function on CPU tensors.  GPU execution is
tests/test_affine_multi_gpu.py's.

Largest ratios seen on the emulator: error over the bar against the dense KKT solve 0.081; nrhs = 1 against adjoint()
over the same bar 0.001."""
import ctypes as C
import os
import subprocess

import pytest

import affine_multi_cases as amc

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
    amc.check_serial(LIB, nx, nu, N, batch, kernel, **opts)


@pytest.mark.parametrize("nx,nu,N,kernel", [(4, 2, 6, "wave<8,4>"), (12, 6, 6, "wave<12,8>"), (56, 22, 3, "pair<56,24>")])
def test_padded_solvers_in_the_callers_dimensions(nx, nu, N, kernel):
    amc.check_padded(LIB, nx, nu, N, kernel)


INITIAL = [(0, "-I")] + [(f, k) for f in (1, 2) for k in amc.isc.G0_KINDS]


@pytest.mark.parametrize("init", [None, "bk"], ids=["default", "bk"])
@pytest.mark.parametrize("frac,kind", INITIAL, ids=[f"nc0={('0', 'nx/2', 'nx')[f]},G0={k}" for f, k in INITIAL])
def test_initial_stage(frac, kind, init):
    amc.check_initial(LIB, frac, kind, init)


@pytest.mark.parametrize("which", ["nx2=0", "one knot", "nu>0"])
def test_terminal_knot_edge_cases(which):
    amc.check_terminal(LIB, which)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_ring_after_two_cycle_appends(family):
    amc.check_ring(LIB, family)


def test_grid_indexing_over_seventy_problems():
    amc.check_grid(LIB)


def test_columns_are_independent_bit_for_bit():
    amc.check_column_independence(LIB)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_one_column_against_the_adjoint(family):
    amc.check_against_adjoint(LIB, family)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_what_must_not_move(family):
    amc.check_untouched(LIB, family)


def test_failed_problem_gets_zero_columns():
    amc.check_failed_problem(LIB)


@pytest.mark.parametrize("what", ["nc", "nth", "legs", "dense", "no backward", "new matrices", "nrhs = 0", "null pointers"])
def test_refusals_leave_everything_alone(what):
    amc.check_refusals(LIB, what)


def test_multi_device_handle_is_refused():
    lib = C.CDLL(LIB)
    lib.emu_set_device_count(2)      # two virtual devices
    try:
        amc.check_refusals(LIB, "multi", devices=(0, 1))
    finally:
        lib.emu_set_device_count(1)


def test_allocation_counts():
    amc.check_allocation(LIB, rounds=20)


def test_rebuild_with_every_service_live():
    amc.check_rebuild_with_services_live(LIB)


@pytest.mark.parametrize("pipeline", [False, True], ids=["plain", "pipelined"])
def test_no_host_synchronisation(pipeline):
    amc.check_no_host_sync(LIB, pipeline=pipeline)


def test_layer_function_on_cpu_tensors():
    amc.check_layer(LIB, "cpu")
