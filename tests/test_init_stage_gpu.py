"""The initial stage over nc0, G0 and GAR_HIP_INIT on the MI355X: tests/init_stage_cases.py's rows on the shipped library.
What only the device shows: the wave-scope Bunch-Kaufman of the fused tail (wave_sync instead of workgroup barriers),
kkt0 laid over the stage's LDS while the wave still holds vx in registers, the __ballot-decided branch per problem,
gar_initial_wave on the packed Vxx record.  One small solver (or two) per case."""
import pytest

import init_stage_cases as ic

pytestmark = pytest.mark.gpu


def report(row, kind, err, exact=None):
    print(f"init-report {row} {kind} oracle {err:.2e} exact {'-' if exact is None else f'{exact:.2e}'}")


@pytest.mark.parametrize("row,kind,init,N", ic.serial_cases(),
                         ids=[f"{r}-{k}-{ic.init_id(i)}-N{N}" for r, k, i, N in ic.serial_cases()])
def test_serial(row, kind, init, N):
    report(f"{row}_N{N}_{ic.init_id(init)}", kind, ic.check_serial_case(row, kind, init, N))


@pytest.mark.parametrize("row,kind,init", ic.leg_cases(),
                         ids=[f"{r}-{k}-{ic.init_id(i)}" for r, k, i in ic.leg_cases()])
def test_leg_mode(row, kind, init):
    report(f"{row}_{ic.init_id(init)}", kind, ic.check_leg_case(row, kind, init))


@pytest.mark.parametrize("row", ic.BATCH_ROWS)
def test_mixed_kinds_in_one_launch(row):
    report(f"B1_{row}", "mixed", ic.check_mixed_batch(row))


@pytest.mark.parametrize("case", list(ic.PIPELINED))
def test_pipelined_schedule(case):
    err, plain = ic.check_pipelined(case)
    report("B2", case, err)
    print(f"init-report B2 {case} pipelined-plain {plain:.2e}")


@pytest.mark.parametrize("kind", ["K5", "K1", "K2"])
@pytest.mark.parametrize("row", ic.BATCH_ROWS)
def test_switch_acts_where_the_closed_form_is_eligible(row, kind):
    err, same_x0 = ic.check_switch(row, kind)
    report(f"B3_{row}_bk", kind, err)
    print(f"init-report B3_{row} {kind} forced factorisation reproduces x0 bit for bit: {same_x0}")


@pytest.mark.parametrize("init", ic.INITS, ids=ic.init_id)
@pytest.mark.parametrize("kind", ic.SERIAL_FOLD_KINDS)
@pytest.mark.parametrize("family", ic.SERIAL_FOLD_FAMILIES)
def test_serial_fold(family, kind, init):
    report(f"P1_{family}_{ic.init_id(init)}", kind, ic.check_serial_fold(kind, init, None, family=family))


@pytest.mark.parametrize("family,gset,kind", ic.golden_cases(), ids=["-".join(c) for c in ic.golden_cases()])
def test_exact_fixture(family, gset, kind):
    ic.check_golden_case(family, gset, kind)
