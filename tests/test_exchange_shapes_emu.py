"""The replica exchange over the world / batch / layer tables of exchange_scenarios.py on the host interpreter, from the SAME kernel
sources as librainbow_hip.so: every row of table A (rb_learner_finish_grads against a float64 fold of given blocks), the refusals,
and the rows of table B (two learn steps against the oracle on the mean gradient) that the interpreter finishes in about a minute
— e-d-w2-b129, e-d-w3-b33 and e-c-w2-hist8 are the device's alone (test_exchange_shapes_gpu.py runs the same bodies on every row)."""
import pytest

import exchange_scenarios as ES
from cabi_adapter import NumpyMem
from guarded_mem import GuardedNumpyMem
from hipemu import loader


@pytest.fixture(scope="module")
def emu():
    return loader.load()


@pytest.mark.parametrize("case", list(ES.FINISH_CASES))
def test_finish_grads_matches_a_float64_fold_of_given_blocks(emu, case):
    ES.check_finish(emu, GuardedNumpyMem, case, where="emu")


def test_exchange_refuses_bad_worlds_idle_handles_and_generic_fc(emu):
    ES.check_refusals(emu, NumpyMem, where="emu")


def test_exchange_refuses_a_layout_with_too_many_norm_partials_when_armed(emu):
    ES.check_slot_limit(emu, NumpyMem, where="emu")


@pytest.mark.parametrize("case,flagset", ES.EMU_LEARN_RUNS, ids=["%s-%s" % r for r in ES.EMU_LEARN_RUNS])
def test_learn_steps_with_the_exchange_armed_match_oracle_on_mean_gradient(emu, case, flagset):
    ES.check_learn(emu, NumpyMem, case, flagset, where="emu")
