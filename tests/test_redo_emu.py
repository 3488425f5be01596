"""Recycling dormant units on the host interpreter: the bodies of tests/redo_scenarios.py (tests/redo_oracle.py has the rules), and
the oracle's own index sets and mask rule against hand-made cases."""
import numpy as np
import pytest

import redo_oracle as RD
import redo_scenarios as R
from cabi_adapter import NumpyMem
from hipemu import loader

ROWS = sorted(R.ROWS)


@pytest.fixture(scope="module")
def emu():
    return loader.load()


# ----------------------------------------------------------------------------------------------------------- oracle --
LAYOUT = {"convs.0.weight": (0, (2, 1, 2, 2)), "convs.0.bias": (64, (2,)), "convs.2.weight": (128, (3, 2, 1, 1)), "convs.2.bias": (192, (3,)),
          "fc_h_v.weight_mu": (256, (2, 6)), "fc_h_v.weight_sigma": (320, (2, 6)), "fc_h_v.bias_mu": (384, (2,)), "fc_h_v.bias_sigma": (448, (2,)),
          "fc_h_a.weight_mu": (268, (2, 6)), "fc_h_a.weight_sigma": (332, (2, 6)), "fc_h_a.bias_mu": (386, (2,)), "fc_h_a.bias_sigma": (450, (2,)),
          "fc_z_v.weight_mu": (512, (2, 2)), "fc_z_v.weight_sigma": (576, (2, 2)), "fc_z_v.bias_mu": (640, (2,)), "fc_z_v.bias_sigma": (704, (2,)),
          "fc_z_a.weight_mu": (516, (4, 2)), "fc_z_a.weight_sigma": (580, (4, 2)), "fc_z_a.bias_mu": (642, (4,)), "fc_z_a.bias_sigma": (706, (4,))}


def test_oracle_index_sets_by_hand():
    """A toy layout (2 and 3 conv channels of P = 2 positions, hidden 2, atoms 2, actions 2) written out by hand."""
    assert RD.unit_layout(LAYOUT) == [("convs.0", 2), ("convs.2", 3), ("fc_h_v", 2), ("fc_h_a", 2)]
    inc, o0, oc = RD.index_sets(LAYOUT, 1)                      # conv 0, channel 1
    assert inc.tolist() == [4, 5, 6, 7, 65] and o0.tolist() == [129, 131, 133] and oc.size == 0
    inc, o0, oc = RD.index_sets(LAYOUT, 2 + 2)                  # the last conv layer's channel 2: columns 4, 5 of all four fc_h rows
    assert inc.tolist() == [132, 133, 194]
    assert o0.tolist() == [260, 261, 266, 267, 272, 273, 278, 279] and oc.tolist() == [324, 325, 330, 331, 336, 337, 342, 343]
    inc, o0, oc = RD.index_sets(LAYOUT, 5 + 1)                  # fc_h_v unit 1
    assert inc.tolist() == list(range(262, 268)) + list(range(326, 332)) + [385, 449]
    assert o0.tolist() == [513, 515] and oc.tolist() == [577, 579]
    inc, o0, oc = RD.index_sets(LAYOUT, 7 + 0)                  # fc_h_a unit 0: rows [Z, NZ) of the output layer
    assert inc.tolist() == list(range(268, 274)) + list(range(332, 338)) + [386, 450]
    assert o0.tolist() == [516, 518, 520, 522] and oc.tolist() == [580, 582, 584, 586]


def test_oracle_zero_wins_and_phi_is_keyed_by_the_element():
    n = 768
    rs = np.random.RandomState(0)
    st = {k: rs.rand(n).astype(np.float32) + 1 for k in "ptmv"}
    mask = np.zeros(9, np.uint8)
    mask[[1, 3]] = 1                                            # conv 0 channel 1 and conv 1 channel 1 meet in element 131
    out, kind, both = RD.recycle(LAYOUT, st, mask, 0.1, 5, 6)
    assert both == 1 and kind[131] == RD.OUTGOING and out["p"][131] == 0.0 and out["m"][131] == 0.0
    phi = RD.phi_flat(LAYOUT, n, 0.1, 5, 6)
    assert out["p"][130] == phi[130] and out["t"][130] == phi[130] and abs(phi[130]) <= 1 / np.sqrt(2.0)
    assert np.array_equal(out["p"][kind == RD.UNTOUCHED], st["p"][kind == RD.UNTOUCHED])
    alone, _, _ = RD.recycle(LAYOUT, st, np.eye(9, dtype=np.uint8)[3], 0.1, 5, 6)
    assert alone["p"][130] == out["p"][130] and alone["p"][131] == phi[131] != 0.0
    assert not np.array_equal(RD.phi_flat(LAYOUT, n, 0.1, 5, 7), phi) and not np.array_equal(RD.phi_flat(LAYOUT, n, 0.1, 4, 6), phi)


def test_oracle_mask_rule_by_hand():
    act = np.array([1.0, 3.0,   0.0, 0.0, 0.0,   np.nan, 2.0,   0.0, 5.0])
    mask, counts, scores = RD.dormant(LAYOUT, act, 0.5)
    assert mask.tolist() == [1, 0,  1, 1, 1,  0, 0,  1, 0] and counts.tolist() == [1, 3, 0, 1]       # 1 * 2 == 0.5 * 4: dormant
    assert scores[:5].tolist() == [0.5, 1.5, 0.0, 0.0, 0.0] and np.isnan(scores[5:7]).all() and scores[7:].tolist() == [0.0, 2.0]
    assert RD.dormant(LAYOUT, act, 0.0)[0].tolist() == [0, 0,  1, 1, 1,  0, 0,  1, 0]


# ----------------------------------------------------------------------------------------------------- kernel level --
@pytest.mark.parametrize("row", sorted(R.RECYCLE_ROWS))
def test_unit_layout_equals_the_oracle(emu, row):
    R.layout_check(emu, NumpyMem, row)


@pytest.mark.parametrize("row", ROWS)
def test_activity_is_the_float64_sum_of_the_activations(emu, row):
    R.activity_check(emu, NumpyMem, row)


def test_measuring_has_no_side_effects(emu):
    R.no_side_effects_check(emu, NumpyMem())


def test_activity_refuses_while_gradients_wait_for_the_exchange(emu):
    R.refusal_check(emu, NumpyMem())


@pytest.mark.parametrize("row", ROWS)
def test_mask_and_counts_equal_the_oracle(emu, row):
    R.mask_check(emu, NumpyMem, row)


@pytest.mark.parametrize("row", sorted(R.RECYCLE_ROWS))
def test_recycle_equals_the_oracle_bit_for_bit(emu, row):
    R.recycle_check(emu, NumpyMem, row)


@pytest.mark.parametrize("row", sorted(R.RECYCLE_ROWS))
def test_recycle_does_not_read_non_finite_parameters(emu, row):
    R.bad_inputs_check(emu, NumpyMem, row)


def test_draw_is_keyed_by_seed_and_draw_only(emu):
    R.keys_check(emu, NumpyMem, "de48")


@pytest.mark.parametrize("row", ROWS)
def test_function_is_preserved_and_units_fire_again(emu, row):
    R.function_preserved_check(emu, NumpyMem, row)


@pytest.mark.parametrize("case", sorted(R.LEARN_CASES))
def test_learning_goes_on_after_a_recycle(emu, case):
    R.learn_check(emu, NumpyMem(), case)


def test_one_call_path_keeps_no_hidden_state(emu):
    R.one_call_check(emu, NumpyMem())
