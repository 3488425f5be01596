"""The vectorised evaluation on the MI355X: the host-interpreter checks of test_eval_emu.py on the device (more rows, more than
one workgroup), and the Python surface: Agent.act_batch(epsilon=...), EpisodeTally, evaluate_vec on the device Catch against
tests/catch_oracle.py and tests/eval_oracle.py, evaluate_host_vec on scripted emulators."""
import types

import numpy as np
import pytest
import torch

import catch_oracle as CO
import eval_oracle as EO
import eval_scenarios as ES
from cabi_adapter import TorchMem

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_STAT = 64
SEED_STAT = ES.pick_seed(N_STAT)             # chosen on the CPU: the oracle explores 20-30 % of the draws checked below


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def ctx(hip):
    c = ES.EpsContext(hip, TorchMem(), N_STAT)
    yield c
    c.close()


# ------------------------------------------------------------------ the emulator's checks on the device
@pytest.mark.parametrize("row0", ES.ROW0S)
@pytest.mark.parametrize("n", [1, 2, 7, 64])
def test_eps_zero_is_greedy_and_eps_one_is_the_oracle_draw_on_device(ctx, n, row0):
    ES.check_eps_zero_and_one(ctx, n, row0)


@pytest.mark.parametrize("row0", ES.ROW0S)
def test_eps_quarter_matches_the_oracle_row_for_row_on_device(ctx, row0):
    ES.check_eps_quarter(ctx, N_STAT, row0, SEED_STAT, range(ES.EPS_ROUNDS))


@pytest.mark.parametrize("n", [2, 64])
def test_eps_draws_replay_and_move_with_the_round_on_device(ctx, n):
    ES.check_eps_replay(ctx, n)


def test_eps_head_refusals_on_device(hip):
    ES.check_eps_refusals(hip, TorchMem())


@pytest.mark.parametrize("S,episodes", [(1, 1), (1, 5), (3, 7), (64, 10), (64, 130)])
def test_tally_matches_the_oracle_on_device(hip, S, episodes):
    ES.check_tally_against_oracle(hip, TorchMem(), S, episodes, seed=200 * S + episodes)


def test_tally_refusals_on_device(hip):
    ES.check_tally_refusals(hip, TorchMem())


# ------------------------------------------------------------------ the Python surface
def _args(**kw):
    base = dict(device=torch.device(DEV), history_length=4, discount=0.99, multi_step=3, priority_weight=0.4,
                priority_exponent=0.5, atoms=51, V_min=-10.0, V_max=10.0, batch_size=32, norm_clip=10.0, model=None,
                learning_rate=1e-4, adam_eps=1.5e-4, architecture="data-efficient", hidden_size=64, noisy_std=0.1,
                replay_frequency=4, target_update=500, learn_start=3200, reward_clip=1)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.fixture(scope="module")
def agent(hip):
    from rainbow_amd.agent import Agent
    torch.manual_seed(3)
    np.random.seed(3)
    return Agent(_args(), types.SimpleNamespace(action_space=lambda: CO.ACTIONS))


def test_act_batch_epsilon_does_not_depend_on_the_chunking(agent):
    """67 states with batch_size = 32: the chunks are 64 + 3.  One call equals the two parts acted on separately (the second
    with row0 = 64), on the host and on the device, and the oracle's draw over the greedy actions."""
    states = torch.from_numpy(ES.varied_states(67, 4, seed=5)).to(DEV)
    agent.train()
    A = CO.ACTIONS
    # a round (picked on the CPU) in which the tail rows 64 .. 66 hold both kinds of row and draw other actions than rows 0 .. 2
    rnd = next(r for r in range(200) if 0 < EO.eps_rows(SEED_STAT, r, 64, 3, 0.5, A)[0].sum() < 3
               and not np.array_equal(EO.eps_rows(SEED_STAT, r, 64, 3, 1.0, A)[1], EO.eps_rows(SEED_STAT, r, 0, 3, 1.0, A)[1]))
    rng = (SEED_STAT, rnd)
    greedy = agent.act_batch(states)
    assert np.array_equal(agent.act_batch(states, epsilon=None, rng=rng), greedy)
    whole = agent.act_batch(states, epsilon=0.5, rng=rng)
    parts = np.concatenate([agent.act_batch(states[:64], epsilon=0.5, rng=rng), agent.act_batch(states[64:], epsilon=0.5, rng=rng, row0=64)])
    assert whole.dtype == np.int64 and np.array_equal(whole, parts)
    on_device = agent.act_batch(states, device_out=True, epsilon=0.5, rng=rng)
    assert on_device.dtype == torch.int32 and on_device.device.type == "cuda" and np.array_equal(on_device.cpu().numpy(), whole)
    want_e, want_a = EO.eps_rows(rng[0], rng[1], 0, 67, 0.5, A)
    assert 15 <= want_e.sum() <= 52
    assert np.array_equal(whole, np.where(want_e == 1, want_a, greedy))
    # the row offset is what carries the tail's draws: without it the three states draw as rows 0 .. 2
    all_explored = agent.act_batch(states, epsilon=1.0, rng=rng)
    assert np.array_equal(all_explored, EO.eps_rows(rng[0], rng[1], 0, 67, 1.0, A)[1])
    unshifted = agent.act_batch(states[64:], epsilon=1.0, rng=rng)
    assert np.array_equal(unshifted, all_explored[:3]) and not np.array_equal(unshifted, all_explored[64:])
    assert np.array_equal(agent.act_batch(states, epsilon=0.0, rng=rng), greedy)
    with pytest.raises(RuntimeError, match="epsilon"):
        agent.act_batch(states, epsilon=-1.0, rng=rng)


def _oracle_evaluation(S, env_seed, episodes, actions_of):
    """test.py:19-34 on the oracle environment with the oracle tally; actions_of(round, stacks) -> S actions."""
    env, tally = CO.CatchOracle(S, 4, env_seed), EO.TallyOracle(S, episodes)
    stacks = env.reset()
    rnd = 0
    while tally.remaining() > 0:
        stacks, rewards, terminals = env.step(actions_of(rnd, stacks))
        tally.step(rewards, ~terminals)
        rnd += 1
    returns, lengths, _ = tally.result()
    return [float(x) for x in returns], [int(x) for x in lengths]


@pytest.mark.parametrize("S,episodes", [(7, 10), (1, 2)])
def test_evaluate_vec_with_epsilon_one_is_the_oracle_episode_list(agent, S, episodes):
    from rainbow_amd.envs import CatchVec
    from rainbow_amd.loop import evaluate_vec
    env_seed, seed = 21, 5
    agent.train()
    out = evaluate_vec(agent, CatchVec(S, DEV, seed=env_seed), episodes, epsilon=1.0, seed=seed)
    assert agent.training                                            # the mode it came in
    want_rewards, want_lengths = _oracle_evaluation(S, env_seed, episodes, lambda r, _: EO.eps_rows(seed, r, 0, S, 1.0, CO.ACTIONS)[1])
    assert out["rewards"] == want_rewards and len(out["rewards"]) == episodes
    assert out["lengths"] == want_lengths == [11] * episodes
    assert set(out["rewards"]) <= {-1.0, 1.0}
    assert out["avg_reward"] == sum(want_rewards) / episodes and out["Qs"] is None and out["avg_Q"] is None
    again = evaluate_vec(agent, CatchVec(S, DEV, seed=env_seed), episodes, epsilon=1.0, seed=seed, poll_every=3)
    assert again == out


def test_evaluate_vec_with_epsilon_zero_is_the_greedy_loop(agent):
    from rainbow_amd.envs import CatchVec
    from rainbow_amd.loop import evaluate_vec
    S, episodes, env_seed = 7, 10, 33
    agent.eval()
    out = evaluate_vec(agent, CatchVec(S, DEV, seed=env_seed), episodes, epsilon=0.0, seed=1)
    assert not agent.training
    greedy = lambda _, stacks: agent.act_batch(torch.from_numpy(stacks).to(DEV))
    want_rewards, want_lengths = _oracle_evaluation(S, env_seed, episodes, greedy)
    assert out["rewards"] == want_rewards and out["lengths"] == want_lengths
    assert evaluate_vec(agent, CatchVec(S, DEV, seed=env_seed), episodes, epsilon=0.0, seed=2) == out      # nothing is drawn


def test_evaluate_vec_raises_when_max_rounds_is_too_small(agent):
    from rainbow_amd.envs import CatchVec
    from rainbow_amd.loop import evaluate_vec
    agent.train()
    with pytest.raises(RuntimeError, match="max_rounds"):
        evaluate_vec(agent, CatchVec(7, DEV, seed=1), 10, epsilon=1.0, max_rounds=21)      # 22 rounds are needed
    assert agent.training
    assert len(evaluate_vec(agent, CatchVec(7, DEV, seed=1), 10, epsilon=1.0, max_rounds=22)["rewards"]) == 10


def test_evaluate_vec_returns_the_validation_q_values(agent):
    from rainbow_amd.envs import CatchVec
    from rainbow_amd.loop import evaluate_vec
    from rainbow_amd.memory import ReplayMemory
    cap = 24
    val = ReplayMemory(_args(), cap, seed=1)
    g = torch.Generator(device="cuda").manual_seed(4)
    frames = torch.randint(0, 256, (cap, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
    val.append_batch(frames, np.full(cap, -1), np.zeros(cap), np.arange(cap) % 9 == 8)
    agent.train()
    out = evaluate_vec(agent, CatchVec(3, DEV, seed=2), 3, val_mem=val)
    agent.eval()
    want = agent.evaluate_q_memory(val)
    agent.train()
    assert len(want) == cap and np.array_equal(np.asarray(out["Qs"]).view(np.uint32), want.view(np.uint32))
    assert out["avg_Q"] == sum(float(q) for q in want) / cap
    assert len(out["rewards"]) == 3


# ------------------------------------------------------------------ the host path
class ScriptedEmu:
    """Stream s: every game lasts 2 + 3 s steps and pays s on its last step."""
    H, W = 12, 16

    def __init__(self, s, lose_life_at=None):
        self.s, self.t, self.games, self.lose_life_at = s, 0, -1, lose_life_at

    def reset(self, out_a):
        self.games += 1
        self.t = 0
        out_a[...] = 10 * self.s + self.games % 7

    def step(self, action, out_a, out_b):
        self.t += 1
        out_a[...] = 40 + self.t
        out_b[...] = 41 + self.t + action
        done = self.t == 2 + 3 * self.s
        return 6, (float(self.s) if done else 0.0), done, self.lose_life_at == self.t


def _host_agent():
    from rainbow_amd.agent import Agent
    torch.manual_seed(5)
    return Agent(_args(batch_size=4, hidden_size=32), types.SimpleNamespace(action_space=lambda: 3))


def test_evaluate_host_vec_gives_every_stream_its_share():
    from rainbow_amd.frames import FrameStackVec
    from rainbow_amd.loop import evaluate_host_vec
    agent = _host_agent()
    agent.train()
    emus = [ScriptedEmu(s) for s in range(3)]
    out = evaluate_host_vec(agent, emus, FrameStackVec(3, DEV, height=ScriptedEmu.H, width=ScriptedEmu.W), 7, epsilon=0.25, seed=3)
    assert agent.training
    assert out["rewards"] == [0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 2.0]          # quotas 3, 2, 2
    assert out["lengths"] == [2, 2, 2, 5, 5, 8, 8]
    assert out["avg_reward"] == 6.0 / 7.0 and out["Qs"] is None
    # what "the first 7 episodes to finish, any stream" would have recorded: the bias this protocol removes
    ends = sorted((k * (2 + 3 * s), s) for s in range(3) for k in range(1, 8))[:7]
    first_come = sorted(float(s) for _, s in ends)
    assert first_come != sorted(out["rewards"]) and sum(first_come) / 7 < out["avg_reward"]
    with pytest.raises(RuntimeError, match="max_rounds"):
        evaluate_host_vec(agent, [ScriptedEmu(s) for s in range(3)], FrameStackVec(3, DEV, height=12, width=16), 7, max_rounds=15)
    with pytest.raises(ValueError, match="life"):
        evaluate_host_vec(agent, [ScriptedEmu(0), ScriptedEmu(1, lose_life_at=2), ScriptedEmu(2)],
                          FrameStackVec(3, DEV, height=12, width=16), 7)
    assert agent.training
    with pytest.raises(ValueError, match="streams"):
        evaluate_host_vec(agent, emus[:2], FrameStackVec(3, DEV, height=12, width=16), 4)


def test_episode_tally_class_against_the_oracle():
    from rainbow_amd.evaluate import EpisodeTally, stream_quotas
    S, E = 5, 12
    assert stream_quotas(S, E).tolist() == EO.quotas(S, E).tolist() == [3, 3, 2, 2, 2]
    tally, ora = EpisodeTally(S, E, DEV), EO.TallyOracle(S, E)
    rs = np.random.RandomState(8)
    for lap in range(2):
        t = 0
        while ora.remaining() > 0:
            t += 1
            rewards, nonterm = ES.scripted_round(rs, S, t)
            # (uint8 flags and bool nonterminals are both accepted)
            flags = torch.from_numpy(nonterm).to(DEV) if t % 2 else torch.from_numpy(nonterm.astype(bool)).to(DEV)
            tally.step(torch.from_numpy(rewards).to(DEV), flags)
            ora.step(rewards, nonterm)
            if t % 4 == 0:
                assert tally.remaining() == ora.remaining()
        assert tally.remaining() == 0 and ES.same_record(tally.result(), ora.result())
        tally.reset()
        ora.reset()
        assert tally.remaining() == E
    with pytest.raises(ValueError, match="streams"):
        tally.step(torch.zeros(4, device=DEV), torch.ones(4, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="episodes"):
        EpisodeTally(S, 0, DEV)
    tally.close()
