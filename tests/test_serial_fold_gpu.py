"""The serial fold (GAR_HIP_SERIAL_FOLD=1) on the MI355X: tests/serial_fold_cases.py's checks on the shipped library.
One or two small solvers per test; the headline-size run is scripts/bench_serial_fold.py's."""
import pytest

from aligator_amd.gar import set_option
import serial_fold_cases as sf

pytestmark = pytest.mark.gpu


def test_the_switch_is_a_known_option():
    set_option("SERIAL_FOLD", "1")
    set_option("SERIAL_FOLD", None)


CASE_FAMILY_MU = [(c, f, mu) for c in "ABCDE" for f in sf.case_families(c) for mu in sf.MUEQS]


@pytest.mark.parametrize("case,family,mueq", CASE_FAMILY_MU)
def test_parity_with_the_oracle(case, family, mueq):
    sf.check_case(case, family, mueq)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_problem_with_D_falls_back_bitwise(family):
    sf.check_fallback_bitwise(None, family)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_mueq_zero_is_reported(family):
    sf.check_mueq_zero(None, family)


def test_serial_fold_agrees_with_leg_fold():
    sf.check_against_leg_fold()


def test_switch_off_is_the_generic_path_bitwise():
    sf.check_switch()


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_cycle_append(family):
    sf.check_cycle_append(None, family)


def test_update_lq_subproblem_device():
    sf.check_update_lq(None, device=True)


def test_pipeline_is_refused():
    sf.check_pipeline_refused()


def test_no_allocation_inside_the_sweep():
    sf.check_no_allocation(None, rounds=20)
