"""The replica exchange over the world / batch / layer tables of exchange_scenarios.py on the MI355X, N learner handles on one
device standing for N replicas (no RCCL): rb_learner_finish_grads against a float64 fold of given rank blocks from world 2 to the
accepted 64, at one and two slabs per rank, partly filled row and column tiles and head shapes other than (51, 6); the refusals;
and two learn steps with the exchange armed against the oracle on the mean gradient along every switch `exch` makes in the
learn plan."""
import pytest

import exchange_scenarios as ES
from cabi_adapter import TorchMem
from guarded_mem import GuardedTorchMem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", list(ES.FINISH_CASES))
def test_finish_grads_matches_a_float64_fold_of_given_blocks_on_device(hip, case):
    ES.check_finish(hip, GuardedTorchMem, case)


def test_exchange_refuses_bad_worlds_idle_handles_and_generic_fc_on_device(hip):
    ES.check_refusals(hip, TorchMem)


def test_exchange_refuses_a_layout_with_too_many_norm_partials_when_armed_on_device(hip):
    ES.check_slot_limit(hip, TorchMem)


@pytest.mark.parametrize("case,flagset", ES.LEARN_RUNS, ids=["%s-%s" % r for r in ES.LEARN_RUNS])
def test_learn_steps_with_the_exchange_armed_match_oracle_on_mean_gradient_on_device(hip, case, flagset):
    ES.check_learn(hip, TorchMem, case, flagset)
