"""The vectorised evaluation pieces on the host interpreter: the e-greedy head (rb_learner_act_batch_eps) and the device-side
episode tally (rb_tally_*), from the SAME kernel sources as librainbow_hip.so.  The device runs the same checks, and the Python
surface built on them (Agent.act_batch(epsilon=...), EpisodeTally, evaluate_vec, evaluate_host_vec), in test_eval_gpu.py.

A forward of 7 states takes the interpreter over a second, so the e-greedy checks are cut into cases of a few forwards each
that share one learner and its greedy actions."""
import pytest

import eval_scenarios as ES
from cabi_adapter import NumpyMem
from hipemu import loader

N_STAT = 7                                   # rows of the epsilon = 0.25 check
SEED_STAT = ES.pick_seed(N_STAT)             # chosen on the CPU: the oracle explores 20-30 % of the draws checked below


@pytest.fixture(scope="module")
def emu():
    return loader.load()


@pytest.fixture(scope="module")
def ctx(emu):
    c = ES.EpsContext(emu, NumpyMem(), N_STAT)
    yield c
    c.close()


@pytest.mark.parametrize("row0", ES.ROW0S)
@pytest.mark.parametrize("n", [1, 2, 7])
def test_eps_zero_is_greedy_and_eps_one_is_the_oracle_draw(ctx, n, row0):
    ES.check_eps_zero_and_one(ctx, n, row0)


@pytest.mark.parametrize("part", range(ES.EPS_ROUNDS // 2))
@pytest.mark.parametrize("row0", ES.ROW0S)
def test_eps_quarter_matches_the_oracle_row_for_row(ctx, row0, part):
    ES.check_eps_quarter(ctx, N_STAT, row0, SEED_STAT, (2 * part, 2 * part + 1))        # 16 values of rng_round, two per case


def test_eps_draws_replay_and_move_with_the_round(ctx):
    ES.check_eps_replay(ctx, 2)


def test_eps_head_refusals(emu):
    ES.check_eps_refusals(emu, NumpyMem())


@pytest.mark.parametrize("S,episodes", [(1, 1), (1, 5), (3, 7), (64, 10), (64, 130)])
def test_tally_matches_the_oracle(emu, S, episodes):
    ES.check_tally_against_oracle(emu, NumpyMem(), S, episodes, seed=100 * S + episodes)


def test_tally_refusals(emu):
    ES.check_tally_refusals(emu, NumpyMem())
