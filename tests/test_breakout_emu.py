"""The device Breakout environment (rb_breakout_*) on the host interpreter, from the SAME kernel sources as librainbow_hip.so,
against tests/breakout_oracle.py; the device runs the same checks in test_breakout_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import breakout_scenarios as BS
from cabi_adapter import CAbiLearnAdapter, NumpyMem
from guarded_mem import GuardedNumpyMem
from hipemu import loader
from oracle import learner_oracle as O
import scenarios

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    return loader.load()


@pytest.mark.parametrize("life_terminals", [0, 1])
@pytest.mark.parametrize("S,history,rounds", [(1, 1, 200), (1, 4, 200), (7, 1, 200), (7, 4, 200), (64, 4, 100)])
def test_breakout_kernel_matches_the_oracle(emu, S, history, rounds, life_terminals):
    BS.check_breakout_against_oracle(emu, NumpyMem(), S, history, seed=1000 * history + 10 * S + life_terminals,
                                     life_terminals=life_terminals, rounds=rounds)


def test_breakout_scripted_policy(emu):
    BS.check_breakout_scripted_policy(emu, NumpyMem(), seed=BS.SCRIPTED_SEED)


@pytest.mark.parametrize("max_steps", [25, 28])
def test_breakout_step_cap(emu, max_steps):
    BS.check_breakout_step_cap(emu, NumpyMem(), seed=5, max_steps=max_steps)


def test_breakout_last_brick_and_refill(emu):
    BS.check_breakout_last_brick_and_refill(emu, NumpyMem())


def test_breakout_corner(emu):
    BS.check_breakout_corner(emu, NumpyMem())


@pytest.mark.parametrize("life_terminals", [0, 1])
def test_breakout_cap_cases(emu, life_terminals):
    BS.check_breakout_cap_cases(emu, NumpyMem(), life_terminals)


def test_breakout_resume_from_get_state(emu):
    BS.check_breakout_resume(emu, NumpyMem())


def test_breakout_set_state_refusals(emu):
    BS.check_breakout_set_state_refusals(emu, NumpyMem())


def test_breakout_seeds_and_refusals(emu):
    BS.check_breakout_seeds_and_refusals(emu, NumpyMem())


def test_breakout_stays_inside_the_callers_buffers(emu):
    BS.check_breakout_guard_bands(emu, GuardedNumpyMem())


def test_breakout_stays_inside_its_state_block():
    env = dict(os.environ, RB_GUARD="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "breakout_guard_run.py"), "emu"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "guard run ok" in p.stdout, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    assert "overwritten guard bands 0" in p.stdout


def test_whole_breakout_round_equals_host_driven_round(emu):
    name = "k10"                 # data-efficient stack, 3 actions, history 4: the smallest learner the emulator tests use
    cfg = O.Config(**scenarios.LEARN_CONFIGS[name])

    def make_learner():
        ad = CAbiLearnAdapter(emu, NumpyMem(), name)
        ad.load(O.init_params(cfg, 31), O.init_params(cfg, 32))
        ad.reset_noise_online(np.random.RandomState(6).randn(O.noise_draw_count(cfg)).astype(np.float32))
        return ad

    BS.check_breakout_device_round(emu, NumpyMem(), make_learner, S=3, rounds=60, seed=BS.ROUND_SEED_EMU)
