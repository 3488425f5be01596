"""Recycling dormant units on the MI355X: the bodies of tests/redo_scenarios.py on the real library (tests/redo_oracle.py has the
rules; the host interpreter runs the same bodies in tests/test_redo_emu.py)."""
import pytest

import redo_scenarios as R

pytestmark = pytest.mark.gpu

ROWS = sorted(R.ROWS)


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib
    return _lib.load()


@pytest.fixture
def Mem():
    from cabi_adapter import TorchMem
    return TorchMem


@pytest.mark.parametrize("row", sorted(R.RECYCLE_ROWS))
def test_unit_layout_equals_the_oracle(hip, Mem, row):
    R.layout_check(hip, Mem, row)


@pytest.mark.parametrize("row", ROWS)
def test_activity_is_the_float64_sum_of_the_activations(hip, Mem, row):
    R.activity_check(hip, Mem, row)


def test_measuring_has_no_side_effects(hip, Mem):
    R.no_side_effects_check(hip, Mem())


def test_activity_refuses_while_gradients_wait_for_the_exchange(hip, Mem):
    R.refusal_check(hip, Mem())


@pytest.mark.parametrize("row", ROWS)
def test_mask_and_counts_equal_the_oracle(hip, Mem, row):
    R.mask_check(hip, Mem, row)


@pytest.mark.parametrize("row", sorted(R.RECYCLE_ROWS))
def test_recycle_equals_the_oracle_bit_for_bit(hip, Mem, row):
    R.recycle_check(hip, Mem, row)


@pytest.mark.parametrize("row", sorted(R.RECYCLE_ROWS))
def test_recycle_does_not_read_non_finite_parameters(hip, Mem, row):
    R.bad_inputs_check(hip, Mem, row)


def test_draw_is_keyed_by_seed_and_draw_only(hip, Mem):
    R.keys_check(hip, Mem, "de48")


@pytest.mark.parametrize("row", ROWS)
def test_function_is_preserved_and_units_fire_again(hip, Mem, row):
    R.function_preserved_check(hip, Mem, row)


@pytest.mark.parametrize("case", sorted(R.LEARN_CASES))
def test_learning_goes_on_after_a_recycle(hip, Mem, case):
    R.learn_check(hip, Mem(), case)


def test_one_call_path_keeps_no_hidden_state(hip, Mem):
    R.one_call_check(hip, Mem())
