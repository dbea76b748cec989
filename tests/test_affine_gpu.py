"""Re-solve for new affine terms (gar_hip_upload_affine, gar_hip_backward_affine) on the MI355X:
tests/affine_cases.py's checks on the shipped library.  Small solvers; the headline-size timing is
scripts/bench_affine_resolve.py's.

Largest ratio of the re-solve over the library's own full solve seen on the GPU (margin 10): distance to the oracle
2.67, KKT triple 0.034."""
import pytest

import affine_cases as ac

pytestmark = pytest.mark.gpu
LIB = None


SERIAL = [(8, 4, 5, 3, "wave<8,4>", dict(BACKWARD="wave")), (8, 4, 5, 3, "mfma<8,4>", dict(BACKWARD="wg4")),
          (36, 12, 4, 2, "wave<36,12>", dict(BACKWARD="wave")), (8, 4, 4, 2, "generic", dict(FORCE_GENERIC="1"))]


@pytest.mark.parametrize("nx,nu,N,batch,kernel,opts", SERIAL, ids=[r[4] for r in SERIAL])
def test_serial_families_three_affine_sets_then_the_original(nx, nu, N, batch, kernel, opts):
    ac.check_serial(LIB, nx, nu, N, batch, kernel, **opts)


@pytest.mark.parametrize("nx,nu,N,kernel", [(4, 2, 6, "wave<8,4>"), (12, 6, 6, "wave<12,8>"), (56, 22, 3, "pair<56,24>")])
def test_padded_solvers_in_the_callers_dimensions(nx, nu, N, kernel):
    ac.check_padded(LIB, nx, nu, N, kernel)


INITIAL = [(0, "-I")] + [(f, k) for f in (1, 2) for k in ac.isc.G0_KINDS]


@pytest.mark.parametrize("init", [None, "bk"], ids=["default", "bk"])
@pytest.mark.parametrize("frac,kind", INITIAL, ids=[f"nc0={('0', 'nx/2', 'nx')[f]},G0={k}" for f, k in INITIAL])
def test_initial_stage(frac, kind, init):
    ac.check_initial(LIB, frac, kind, init)


@pytest.mark.parametrize("which", ["nx2=0", "one knot", "nu>0"])
def test_terminal_knot_edge_cases(which):
    ac.check_terminal(LIB, which)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_ring_after_two_cycle_appends(family):
    ac.check_ring(LIB, family)


def test_grid_indexing_over_seventy_problems():
    ac.check_grid(LIB)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_what_must_not_move(family):
    ac.check_untouched(LIB, family)


def test_new_matrices_invalidate_until_the_next_backward():
    ac.check_invalidation(LIB)


@pytest.mark.parametrize("what", ["nc", "nth", "legs", "dense", "no backward"])
def test_refusals_leave_the_records_alone(what):
    ac.check_refusals(LIB, what)


def test_multi_device_handle_is_refused():
    ac.check_refusals(LIB, "multi", devices=(0, 0))     # the same device twice


def test_failed_problem_is_left_alone():
    ac.check_failed_problem(LIB)


def test_allocation_counts():
    ac.check_allocation(LIB, rounds=20)


@pytest.mark.parametrize("pipeline", [False, True], ids=["plain", "pipelined"])
def test_no_host_synchronisation(pipeline):
    ac.check_no_host_sync(LIB, pipeline=pipeline)


def test_the_librarys_pipelined_default_batch():
    ac.check_default_batch()
