"""What a caller reads back while cached results are in play (gar_hip_backward_blocks' eager roll-out,
gar_hip_prefetch_gains, gar_hip_collapse_feedback, gar_hip_backward_affine, gar_hip_cycle_append) on the emulator:
tests/run_state_cases.py's scenarios on the CPU build of the unmodified sources (tests/emu).  The emulator executes
streams synchronously: these are the state rules of DESIGN.md 1b; the ordering of the copies on the second stream is
tests/test_run_state_gpu.py's."""
import os
import subprocess

import pytest

import run_state_cases as rs

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "emu", "_build", "libgar_hip_emu.so")


@pytest.fixture(scope="module", autouse=True)
def build_emu():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu")], check=True)


@pytest.mark.parametrize("n,shape", rs.CASES, ids=rs.IDS)
def test_cached_results_equal_the_uncached_sequence_bit_for_bit(n, shape):
    rs.check_scenario(LIB, n, shape)


def test_refusal_texts_of_backward_affine_and_refine():
    rs.check_refusal_texts(LIB)
