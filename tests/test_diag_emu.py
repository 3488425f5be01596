"""Device-side diagnostics (step records, held-out loss, priority statistics) on the host interpreter, from the SAME kernel
sources as librainbow_hip.so: the bodies of diag_scenarios.py.  The device runs them in test_diag_gpu.py."""
import pytest

import diag_scenarios as DS
from cabi_adapter import NumpyMem
from hipemu import loader


@pytest.fixture(scope="module")
def emu():
    return loader.load()


@pytest.mark.parametrize("case", sorted(DS.EMU_CASES) + [DS.EMU_B33_CASE])
def test_step_records_eager_path(emu, case):
    DS.check_records_eager(emu, NumpyMem(), case)


@pytest.mark.parametrize("case", sorted(DS.EMU_CASES))
def test_step_records_one_call_path(emu, case):
    DS.check_records_one_call(emu, NumpyMem(), case)


def test_ring_wraps(emu):
    DS.check_ring_wraps(emu, NumpyMem())


def test_failed_draw_is_recorded_and_does_not_advance_the_step(emu):
    DS.check_failed_draw(emu, NumpyMem())


def test_exchange_leaves_no_norm_and_blocks_eval_loss(emu):
    DS.check_exchange_gives_nan(emu, NumpyMem())


def test_records_are_deterministic_and_the_off_switch_changes_nothing(emu):
    DS.check_deterministic_and_off(emu, NumpyMem(), count_launches=False, case="z51-a6", steps=1)


@pytest.mark.parametrize("case", sorted(DS.EMU_CASES) + [DS.EMU_B33_CASE])
def test_eval_loss_matches_the_oracle(emu, case):
    DS.check_eval_loss(emu, NumpyMem(), case)


def test_eval_loss_has_no_side_effects(emu):
    DS.check_eval_no_side_effects(emu, NumpyMem())


def test_eval_loss_and_set_stats_refuse_bad_arguments(emu):
    DS.check_eval_refusals(emu, NumpyMem())


@pytest.mark.parametrize("state", DS.PSTATS_STATES)
@pytest.mark.parametrize("capacity", DS.PSTATS_CAPACITIES)
def test_priority_stats(emu, capacity, state):
    DS.check_priority_stats(emu, NumpyMem(), capacity, state)


def test_priority_stats_refuses_null(emu):
    DS.check_priority_stats_refusals(emu, NumpyMem())
