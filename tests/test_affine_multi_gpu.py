"""A resident batch solved for many affine terms at once (gar_hip_affine_solve_multi, gar_hip_affine_solve_multi_async,
aligator_amd/layer.py: lq_affine_solve_multi) on the MI355X: tests/affine_multi_cases.py's checks on the shipped library,
the layer function on cuda tensors.  Small solvers; the headline-size timing is scripts/bench_affine_multi.py's.

Largest ratios seen on the GPU: error over the bar against the dense KKT solve 0.085; nrhs = 1 against adjoint() over
the same bar 0.000."""
import pytest

import affine_multi_cases as amc

pytestmark = pytest.mark.gpu
LIB = None


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
    amc.check_refusals(LIB, "multi", devices=(0, 0))     # the same device twice


def test_allocation_counts():
    amc.check_allocation(LIB, rounds=20)


def test_rebuild_with_every_service_live():
    amc.check_rebuild_with_services_live(LIB)


@pytest.mark.parametrize("pipeline", [False, True], ids=["plain", "pipelined"])
def test_no_host_synchronisation(pipeline):
    amc.check_no_host_sync(LIB, pipeline=pipeline)


def test_layer_function_on_cuda_tensors():
    amc.check_layer(LIB, "cuda")
