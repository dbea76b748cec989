"""Gradients of a resident batch (gar_hip_adjoint, gar_hip_adjoint_async, gar_hip_upload_packed_user_device,
gar_hip_solution_vectors_device, aligator_amd/layer.py) on the MI355X: tests/adjoint_cases.py's checks on the shipped
library, the PyTorch layer on cuda tensors.  Small solvers; the headline-size timing is scripts/bench_adjoint.py's.

Largest ratios seen on the GPU: adjoint over the library's full solve of the substituted problem (margin 10) 4.03;
gradient entries over their bound 4 eps (|ab| + |cd|) 0.250; gradient against autograd over its bar 0.001."""
import pytest

import adjoint_cases as adc

pytestmark = pytest.mark.gpu
LIB = None


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
    adc.check_refusals(LIB, "multi", devices=(0, 0))     # the same device twice


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


def test_layer_on_cuda_tensors():
    adc.check_layer(LIB, "cuda")
