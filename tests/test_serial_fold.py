"""The serial fold (GAR_HIP_SERIAL_FOLD=1) on the emulator and through the ABI: tests/serial_fold_cases.py's checks on the
CPU build of the unmodified kernel sources (tests/emu).  Index maps of the fold's packed output, of the expand step's
fbT2 / packed-Vxx input, the two layouts and the per-problem fallback are checked here; GPU execution is
tests/test_serial_fold_gpu.py's.  Case E, (56, 24) on pair<>, runs here too: the emulator hosts 128-thread blocks."""
import os
import subprocess

import pytest

from aligator_amd.gar import set_option
import serial_fold_cases as sf

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "_build", "libgar_hip_emu.so")


@pytest.fixture(scope="module", autouse=True)
def build_emu():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu")], check=True)


def test_the_switch_is_a_known_option():
    set_option("SERIAL_FOLD", "1", EMU)
    set_option("SERIAL_FOLD", None, EMU)


CASE_FAMILY_MU = [(c, f, mu) for c in "ABCDE" for f in sf.case_families(c) for mu in sf.MUEQS]


@pytest.mark.parametrize("case,family,mueq", CASE_FAMILY_MU)
def test_parity_with_the_oracle(case, family, mueq):
    sf.check_case(case, family, mueq, EMU)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_problem_with_D_falls_back_bitwise(family):
    sf.check_fallback_bitwise(EMU, family)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_mueq_zero_is_reported(family):
    sf.check_mueq_zero(EMU, family)


def test_serial_fold_agrees_with_leg_fold():
    sf.check_against_leg_fold(EMU)


def test_switch_off_is_the_generic_path_bitwise():
    sf.check_switch(EMU)


@pytest.mark.parametrize("family", ["wave", "wg4"])
def test_cycle_append(family):
    sf.check_cycle_append(EMU, family)


def test_update_lq_subproblem_device():
    sf.check_update_lq(EMU, device=False)


def test_pipeline_is_refused():
    sf.check_pipeline_refused(EMU)


def test_no_allocation_inside_the_sweep():
    sf.check_no_allocation(EMU, rounds=3)
