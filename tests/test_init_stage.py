"""The initial stage over nc0, G0 and GAR_HIP_INIT on the emulator: tests/init_stage_cases.py's rows on the CPU build of the
unmodified kernel sources (tests/emu).  This keeps the table honest -- index maps, the padded [G0 0; 0 -I], the branch
per problem, the deferred initial stage of the pipelined schedule; what the emulator cannot see (wave-scope
synchronisation, LDS overlays, register values carried into the tail) is tests/test_init_stage_gpu.py's.

The lane-per-thread emulator pays seconds for what the device does in microseconds: the whole matrix costs 16 CPU
minutes here and 4 s on the GPU.  So the GPU file runs every (row, kind, switch) combination, and this file runs by
default a cut that keeps every row and every code path the switch or the kind selects -- per serial row a partial
general G0 and +I under the default, -I under GAR_HIP_INIT=bk (the forced factorisation), the free initial state where
it is an edge of its own (dummy rows only on the padded row, nx0 != nx), N = 1 and 2 where the row has them; one kind
per leg row; one batch row of each batch check -- about 3 CPU minutes.  GAR_TESTS_INIT_FULL=1 runs the whole matrix
here too (it passes: DESIGN.md 2b has its figures)."""
import os
import subprocess

import pytest

import init_stage_cases as ic

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu", "_build", "libgar_hip_emu.so")
FULL = os.environ.get("GAR_TESTS_INIT_FULL") == "1"

LEG_KIND = {"L1": "K1", "L2": "K1", "L3": "K0", "L4": "K1", "L5": "K4", "L6a": "K0", "L6b": "K1"}
DENSE_FIXTURE = (("plain", "K3"), ("padded", "K0"), ("cstr", "K1"))


def _serial(row, kind, init, N):
    if N != ic.SERIAL_ROWS[row]["N"]:                       # the horizon-parity cases
        return init is None
    if kind == "K0":
        return init is None and row in ("S1", "S3", "S8")
    return (kind in ("K1", "K3") and init is None) or (kind == "K5" and init == "bk")


def _fixture(family, gset, kind):
    if family == "dense":
        return (gset, kind) in DENSE_FIXTURE
    return family != "leg2" or kind in ("K1", "K3")


SERIAL = [c for c in ic.serial_cases() if FULL or _serial(*c)]
LEGS = [c for c in ic.leg_cases() if FULL or (c[2] is None and c[1] == LEG_KIND[c[0]])]
BATCH = ic.BATCH_ROWS if FULL else ("S1",)
PIPELINED = list(ic.PIPELINED) if FULL else ["partial"]
SWITCH = [(r, k) for r in ic.BATCH_ROWS for k in ("K5", "K1", "K2")] if FULL else [("S1", "K5"), ("S2", "K2")]
FOLD = [(f, k, i) for f in ic.SERIAL_FOLD_FAMILIES for k in ic.SERIAL_FOLD_KINDS for i in ic.INITS
        if FULL or (k == "K1" and i is None)]
FIXTURE = [c for c in ic.golden_cases() if FULL or _fixture(*c)]


@pytest.fixture(scope="module", autouse=True)
def build_emu():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu")], check=True)


def report(row, kind, err, exact=None):
    print(f"init-report {row} {kind} oracle {err:.2e} exact {'-' if exact is None else f'{exact:.2e}'}")


def test_every_row_runs_here():
    assert {c[0] for c in SERIAL} == set(ic.SERIAL_ROWS) and {c[0] for c in LEGS} == set(ic.LEG_ROWS)
    assert {c[0] for c in FIXTURE} == set(ic.GOLDEN_FAMILIES) and {c[1] for c in FIXTURE} == set(ic.GOLDEN_SETS)


@pytest.mark.parametrize("row,kind,init,N", SERIAL, ids=[f"{r}-{k}-{ic.init_id(i)}-N{N}" for r, k, i, N in SERIAL])
def test_serial(row, kind, init, N):
    report(f"{row}_N{N}_{ic.init_id(init)}", kind, ic.check_serial_case(row, kind, init, N, EMU))


@pytest.mark.parametrize("row,kind,init", LEGS, ids=[f"{r}-{k}-{ic.init_id(i)}" for r, k, i in LEGS])
def test_leg_mode(row, kind, init):
    report(f"{row}_{ic.init_id(init)}", kind, ic.check_leg_case(row, kind, init, EMU))


@pytest.mark.parametrize("row", BATCH)
def test_mixed_kinds_in_one_launch(row):
    report(f"B1_{row}", "mixed", ic.check_mixed_batch(row, EMU))


@pytest.mark.parametrize("case", PIPELINED)
def test_pipelined_schedule(case):
    err, plain = ic.check_pipelined(case, EMU)
    report("B2", case, err)
    print(f"init-report B2 {case} pipelined-plain {plain:.2e}")


@pytest.mark.parametrize("row,kind", SWITCH, ids=[f"{r}-{k}" for r, k in SWITCH])
def test_switch_acts_where_the_closed_form_is_eligible(row, kind):
    err, same_x0 = ic.check_switch(row, kind, EMU)
    report(f"B3_{row}_bk", kind, err)
    print(f"init-report B3_{row} {kind} forced factorisation reproduces x0 bit for bit: {same_x0}")


@pytest.mark.parametrize("family,kind,init", FOLD, ids=[f"{f}-{k}-{ic.init_id(i)}" for f, k, i in FOLD])
def test_serial_fold(family, kind, init):
    report(f"P1_{family}_{ic.init_id(init)}", kind, ic.check_serial_fold(kind, init, EMU, family=family))


def test_fixture_pins_the_oracle():
    """the oracle against the 50-digit solutions: the figures the bars of test_exact_fixture are made of"""
    for family, gset, kind in ic.golden_cases():
        _, _, errs = ic.golden_bar(family, gset, kind)
        print(f"init-report X1_{family}-oracle_{gset} {kind} oracle - exact {max(errs):.2e}")
        # unconstrained: well conditioned, a few ulps; constrained at mueq = 1e-6: cond ~ 1 / mueq, eps / mueq = 2e-10
        constrained = ic.GOLDEN_SETS[gset][2] > 0
        assert max(errs) <= (10 * 2.2e-16 / ic.GOLDEN_MUEQ if constrained else 1e-12), (family, gset, kind, errs)


@pytest.mark.parametrize("family,gset,kind", FIXTURE, ids=["-".join(c) for c in FIXTURE])
def test_exact_fixture(family, gset, kind):
    ic.check_golden_case(family, gset, kind, EMU)
