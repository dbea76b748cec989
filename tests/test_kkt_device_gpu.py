"""Device-side KKT residuals and per-problem status (gar_hip_kkt_error, gar_hip_get_status) on the MI355X:
tests/kkt_device_cases.py's checks on the shipped library.  One or two small solvers per test; the headline-size timing
is scripts/bench_kkt_device.py's."""
import numpy as np
import pytest

import kkt_device_cases as kc

pytestmark = pytest.mark.gpu
LIB = None

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
    kc.check_multi_device(LIB, devices=(0, 0))     # the same device twice


def test_the_librarys_pipelined_default_batch():
    """(36, 12), N = 16, batch 8 x #CUs: the batch at which a new solver starts pipelined.  Generated on the device, swept
    and evaluated with no host synchronisation in between; five problems spread over the batch against the host, the
    rest only for dualErr below ten times the largest (host dualErr + bound) the five showed -- a sanity cap, not a
    parity claim."""
    import torch
    from aligator_amd import synth_device
    from aligator_amd.gar import BatchedRiccatiSolver
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nx, nu, N, batch, mueq = 36, 12, 16, 8 * cus, 1e-10
    dims = [(nx, nu, 0, nx, 0)] * N + [(nx, 0, 0, nx, 0)]
    s = BatchedRiccatiSolver(dims, nx, batch=batch)
    assert s.pipeline == 2 and s.kernel_name == "wave<36,12>"
    synth_device.fill_problems(s, seed=11, mode="W")
    s.backward_async(mueq)
    s.forward_async()
    s.kkt_error_async(mueq)
    s.sync()
    assert s.num_failed() == 0 and not s.status().any()
    err, st = kc.device_results(s, None)
    cap = 0.0
    for b in (0, 1, batch // 2 - 1, batch // 2, batch - 1):
        prob, sol = kc.host_problem(s, b), s.solution(b)
        norms, S, n = kc.stage_residuals(prob, sol, mueq)
        bound = 2.0 * n[:, None] * kc.EPS * S
        assert (np.abs(st[b] - norms) <= bound).all(), b
        assert err[b, 2] == st[b, :, 2:].max() and err[b, 0] == st[b, :, 0].max()
        cap = max(cap, float(norms[:, 2:].max() + bound[:, 2:].max()))
    print(f"dualErr: max over the batch {err[:, 2].max():.3e}, cap {10 * cap:.3e}")
    assert np.isfinite(err).all() and (err[:, 2] <= 10.0 * cap).all()
    s.close()
