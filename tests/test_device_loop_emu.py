"""The device-resident actor loop on the host interpreter: the device-operand append round (rb_replay_append_streams_dev), the
device Catch environment (rb_catch_*) and a whole act -> step -> append round, from the SAME kernel sources as
librainbow_hip.so.  The device runs the same checks in test_device_loop_gpu.py."""
import numpy as np
import pytest

import device_loop_scenarios as DS
from cabi_adapter import CAbiLearnAdapter, NumpyMem
from hipemu import loader
from oracle import learner_oracle as O
import scenarios


@pytest.fixture(scope="module")
def emu():
    return loader.load()


@pytest.mark.parametrize("S", [1, 2, 7, 16, 64])
def test_device_operand_round_equals_host_operand_round(emu, S):
    DS.check_append_dev_equals_host(emu, NumpyMem(), S, seed=300 + S)


def test_device_operand_round_refusals(emu):
    DS.check_append_dev_refusals(emu, NumpyMem())


@pytest.mark.parametrize("history", [1, 4])
@pytest.mark.parametrize("S", [1, 7, 64])
def test_catch_kernel_matches_the_oracle(emu, S, history):
    DS.check_catch_against_oracle(emu, NumpyMem(), S, history, seed=1000 * history + S)


def test_catch_seeds_and_refusals(emu):
    DS.check_catch_seeds_and_refusals(emu, NumpyMem())


def test_random_policy_is_poor(emu):
    DS.check_random_policy_is_poor(emu, NumpyMem())


def test_whole_device_round_equals_host_driven_round(emu):
    name = "k10"                 # data-efficient stack, 3 actions, history 4: the smallest learner the emulator tests use
    cfg = O.Config(**scenarios.LEARN_CONFIGS[name])

    def make_learner():
        ad = CAbiLearnAdapter(emu, NumpyMem(), name)
        ad.load(O.init_params(cfg, 31), O.init_params(cfg, 32))
        ad.reset_noise_online(np.random.RandomState(6).randn(O.noise_draw_count(cfg)).astype(np.float32))
        return ad

    DS.check_device_round(emu, NumpyMem(), make_learner)
