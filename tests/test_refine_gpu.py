"""Iterative refinement from the stored factorisation (gar_hip_refine, gar_hip_refine_async) on the MI355X:
tests/refine_cases.py's checks on the shipped library.  Small solvers; the headline-size timing is
scripts/bench_refine.py's.

Largest ratio of the device's step over the oracle's step seen on the GPU (margin 10): KKT triple 0.013, distance to
the oracle's full solve 3.67; of a step from an O(1) residual over the library's full solve: KKT triple 0.394, distance
3.73."""
import pytest

import refine_cases as rc

pytestmark = pytest.mark.gpu
LIB = None


SERIAL = [(8, 4, 5, 3, "wave<8,4>", dict(BACKWARD="wave")), (8, 4, 5, 3, "mfma<8,4>", dict(BACKWARD="wg4")),
          (36, 12, 4, 2, "wave<36,12>", dict(BACKWARD="wave")), (8, 4, 4, 2, "generic", dict(FORCE_GENERIC="1"))]


@pytest.mark.parametrize("nx,nu,N,batch,kernel,opts", SERIAL, ids=[r[4] for r in SERIAL])
def test_serial_families_one_step_then_a_second(nx, nu, N, batch, kernel, opts):
    rc.check_serial(LIB, nx, nu, N, batch, kernel, **opts)


def test_a_step_improves_where_there_is_something_to_improve():
    rc.check_improves(LIB)


@pytest.mark.parametrize("nx,nu,N,kernel", [(4, 2, 6, "wave<8,4>"), (12, 6, 6, "wave<12,8>"), (56, 22, 3, "pair<56,24>")])
def test_padded_solvers_in_the_callers_dimensions(nx, nu, N, kernel):
    rc.check_padded(LIB, nx, nu, N, kernel)


INITIAL = [(0, "-I")] + [(f, k) for f in (1, 2) for k in rc.isc.G0_KINDS]


@pytest.mark.parametrize("init", [None, "bk"], ids=["default", "bk"])
@pytest.mark.parametrize("frac,kind", INITIAL, ids=[f"nc0={('0', 'nx/2', 'nx')[f]},G0={k}" for f, k in INITIAL])
def test_initial_stage(frac, kind, init):
    rc.check_initial(LIB, frac, kind, init)


@pytest.mark.parametrize("which", ["nx2=0", "one knot", "nu>0"])
def test_terminal_knot_edge_cases(which):
    rc.check_terminal(LIB, which)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_ring_after_two_cycle_appends(family):
    rc.check_ring(LIB, family)


def test_grid_indexing_over_seventy_problems():
    rc.check_grid(LIB)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_what_must_not_move(family):
    rc.check_untouched(LIB, family)


def test_threshold_gates_on_the_device():
    rc.check_gate(LIB)


def test_kkt_buffers_describe_the_refined_solution():
    rc.check_kkt_buffers(LIB)


def test_host_copy_of_backward_blocks_is_dropped():
    rc.check_host_copy_dropped(LIB)


def test_refine_after_a_re_solve():
    rc.check_after_resolve(LIB)


def test_new_matrices_invalidate_until_the_next_backward():
    rc.check_invalidation(LIB)


@pytest.mark.parametrize("what", ["nc", "nth", "legs", "dense", "no backward", "no forward", "bad arguments"])
def test_refusals_leave_everything_alone(what):
    rc.check_refusals(LIB, what)


def test_multi_device_handle_is_refused():
    rc.check_refusals(LIB, "multi", devices=(0, 0))     # the same device twice


def test_failed_problem_is_left_alone():
    rc.check_failed_problem(LIB)


def test_allocation_counts():
    rc.check_allocation(LIB, rounds=20)


@pytest.mark.parametrize("pipeline", [False, True], ids=["plain", "pipelined"])
def test_no_host_synchronisation(pipeline):
    rc.check_no_host_sync(LIB, pipeline=pipeline)


def test_the_librarys_pipelined_default_batch():
    rc.check_default_batch()
