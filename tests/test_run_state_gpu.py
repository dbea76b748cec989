"""What a caller reads back while cached results are in play (gar_hip_backward_blocks' eager roll-out,
gar_hip_prefetch_gains, gar_hip_collapse_feedback, gar_hip_backward_affine, gar_hip_cycle_append) on the MI355X:
tests/run_state_cases.py's scenarios on the shipped library -- the state rules of DESIGN.md 1b and, with real
asynchronous copies on the second stream, their ordering."""
import pytest

import run_state_cases as rs

pytestmark = pytest.mark.gpu
LIB = None


@pytest.mark.parametrize("n,shape", rs.CASES, ids=rs.IDS)
def test_cached_results_equal_the_uncached_sequence_bit_for_bit(n, shape):
    rs.check_scenario(LIB, n, shape)


def test_refusal_texts_of_backward_affine_and_refine():
    rs.check_refusal_texts(LIB)
