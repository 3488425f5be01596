"""Feature rank and per-tensor norms on the host interpreter: the bodies of tests/rank_scenarios.py (its docstring has the
tolerances), and the host-side spectrum (rainbow_amd/feature_rank.py), which needs no kernel at all.  The interpreter runs every
Gram shape: the longest, (40, 1024, 1024), is one workgroup and takes seconds."""
import pytest

import rank_scenarios as K
import redo_scenarios as RS
from cabi_adapter import NumpyMem
from hipemu import loader

ROWS = sorted(RS.ROWS)


@pytest.fixture(scope="module")
def emu():
    return loader.load()


# --------------------------------------------------------------------------------------------------------- spectrum --
@pytest.mark.parametrize("n,d", K.SPECTRUM_SHAPES)
def test_spectrum_of_a_planted_matrix(n, d):
    K.spectrum_check(n, d)


def test_spectrum_edges():
    K.spectrum_edges_check()


# ----------------------------------------------------------------------------------------------------- kernel level --
@pytest.mark.parametrize("shape", K.GRAM_SHAPES, ids=lambda s: "n%d-d%d-ld%d" % s)
def test_gram_is_inside_the_bound_of_the_exact_sum(emu, shape):
    K.gram_check(emu, NumpyMem, shape)


def test_gram_bits(emu):
    K.gram_bits_check(emu, NumpyMem)


def test_gram_refusals(emu):
    K.gram_refusals_check(emu, NumpyMem)


@pytest.mark.parametrize("n,d", K.SPECTRUM_SHAPES)
def test_planted_ranks_through_the_device_gram(emu, n, d):
    K.end_to_end_check(emu, NumpyMem, n, d)


@pytest.mark.parametrize("row", ROWS)
def test_captured_rows_equal_debug_read(emu, row):
    K.capture_check(emu, NumpyMem, row)


def test_measuring_has_no_side_effects(emu):
    K.no_side_effects_check(emu, NumpyMem())


def test_capture_refuses_while_gradients_wait_for_the_exchange(emu):
    K.refusal_check(emu, NumpyMem())


@pytest.mark.parametrize("row", ROWS)
def test_tensor_norms_equal_the_reference(emu, row):
    K.norms_check(emu, NumpyMem, row)


@pytest.mark.parametrize("row", ROWS)
def test_tensor_sums_add_up_to_the_learners_gradient_norm(emu, row):
    K.grad_norm_check(emu, NumpyMem(), row)
