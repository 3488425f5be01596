"""The device Breakout environment on the MI355X: the host-interpreter checks of test_breakout_emu.py on the device, and the
Python surface: BreakoutVec through the reference's Env surface, train_device (life-loss terminals, reward clipping, no
synchronisation), evaluate_vec (episodes of varying length) and state_dict round trips, all against tests/breakout_oracle.py.
There is NO learning check here."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import breakout_oracle as BO
import breakout_scenarios as BS
import device_loop_scenarios as DS
import eval_oracle as EO
import scenarios
from cabi_adapter import CAbiLearnAdapter, TorchMem
from guarded_mem import GuardedTorchMem
from oracle import learner_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib as L
    return L.load()


# ------------------------------------------------------------------ the emulator's checks on the device
@pytest.mark.parametrize("life_terminals", [0, 1])
@pytest.mark.parametrize("S,history,rounds", [(1, 1, 200), (1, 4, 200), (7, 1, 200), (7, 4, 200), (64, 4, 100)])
def test_breakout_kernel_matches_the_oracle_on_device(hip, S, history, rounds, life_terminals):
    BS.check_breakout_against_oracle(hip, TorchMem(), S, history, seed=2000 * history + 10 * S + life_terminals,
                                     life_terminals=life_terminals, rounds=rounds)


def test_breakout_scripted_policy_on_device(hip):
    BS.check_breakout_scripted_policy(hip, TorchMem(), seed=BS.SCRIPTED_SEED)


@pytest.mark.parametrize("max_steps", [25, 28])
def test_breakout_step_cap_on_device(hip, max_steps):
    BS.check_breakout_step_cap(hip, TorchMem(), seed=5, max_steps=max_steps)


def test_breakout_last_brick_and_refill_on_device(hip):
    BS.check_breakout_last_brick_and_refill(hip, TorchMem())


def test_breakout_corner_on_device(hip):
    BS.check_breakout_corner(hip, TorchMem())


@pytest.mark.parametrize("life_terminals", [0, 1])
def test_breakout_cap_cases_on_device(hip, life_terminals):
    BS.check_breakout_cap_cases(hip, TorchMem(), life_terminals)


def test_breakout_resume_from_get_state_on_device(hip):
    BS.check_breakout_resume(hip, TorchMem())


def test_breakout_set_state_refusals_on_device(hip):
    BS.check_breakout_set_state_refusals(hip, TorchMem())


def test_breakout_seeds_and_refusals_on_device(hip):
    BS.check_breakout_seeds_and_refusals(hip, TorchMem())


def test_breakout_stays_inside_the_callers_buffers_on_device(hip):
    BS.check_breakout_guard_bands(hip, GuardedTorchMem())


def test_breakout_stays_inside_its_state_block_on_device():
    env = dict(os.environ, RB_GUARD="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "breakout_guard_run.py"), "hip"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "guard run ok" in p.stdout, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    assert "overwritten guard bands 0" in p.stdout


def test_whole_breakout_round_equals_host_driven_round_on_device(hip):
    name = "k10"
    cfg = O.Config(**scenarios.LEARN_CONFIGS[name])

    def make_learner():
        ad = CAbiLearnAdapter(hip, TorchMem(), name)
        ad.load(O.init_params(cfg, 31), O.init_params(cfg, 32))
        ad.reset_noise_online(np.random.RandomState(6).randn(O.noise_draw_count(cfg)).astype(np.float32))
        return ad

    BS.check_breakout_device_round(hip, TorchMem(), make_learner, S=16, rounds=80, seed=BS.ROUND_SEED_GPU)


# ------------------------------------------------------------------ the Python surface
def _args(**kw):
    base = dict(device=torch.device(DEV), history_length=4, discount=0.99, multi_step=3, priority_weight=0.4,
                priority_exponent=0.5, atoms=51, V_min=-10.0, V_max=10.0, batch_size=32, norm_clip=10.0, model=None,
                learning_rate=1e-4, adam_eps=1.5e-4, architecture="data-efficient", hidden_size=64, noisy_std=0.1,
                replay_frequency=4, target_update=500, learn_start=3200, reward_clip=1)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("training", [True, False])
def test_single_stream_env_surface_matches_the_oracle(training):
    """BreakoutVec(streams=1) through the reference's Env surface (reset / step(int) / reset after done) against BreakoutEnv:
    in training mode a lost life is a done whose reset() hands out the stack that moved on, in evaluation mode it is not a done."""
    from rainbow_amd.envs import BreakoutVec
    env, ora = BreakoutVec(1, DEV, seed=44, max_steps=60, training=not training), BO.BreakoutEnv(44, max_steps=60)
    (env.train if training else env.eval)()
    (ora.train if training else ora.eval)()
    assert env.training == training and env.action_space() == ora.action_space() == 3 and env.reward_range == (0.0, 4.0)
    rs = np.random.RandomState(2)
    done, dones, life_dones = True, 0, 0
    for t in range(150):
        if done:
            s, so = env.reset(), ora.reset()
            assert np.array_equal(s.cpu().numpy(), so.numpy()), t
        a = int(rs.randint(0, 3))
        (s, r, done), (so, ro, do) = env.step(a), ora.step(a)
        assert (r, done) == (ro, do) and np.array_equal(s.cpu().numpy(), so.numpy()), t
        dones += done
        life_dones += done and not ora.core.events[0]["over"]
    st = env.stats()
    assert {k: st[k] for k in BO.TOTALS} == ora.core.stats() and st["games"] >= 3 and st["steps"] == 150
    assert (life_dones >= 3 and dones == life_dones + st["games"]) if training else (life_dones == 0 and dones == st["games"])
    assert st["lives_lost"] >= 3
    env.close()


def _run_train(seed, T_max, sync_debug=False):
    from rainbow_amd.agent import Agent
    from rainbow_amd.envs import BreakoutVec
    from rainbow_amd.loop import train_device
    from rainbow_amd.memory import ReplayMemory
    args = _args()
    torch.manual_seed(seed)
    np.random.seed(seed)
    env = BreakoutVec(16, args.device, seed=seed, history_length=args.history_length)
    agent = Agent(args, env)
    mem = ReplayMemory(args, 6400, seed=seed, streams=16)            # 4800 transitions: the ring does not wrap
    if sync_debug:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
    try:
        learns = train_device(agent, mem, env, args, T_max)
    finally:
        if sync_debug:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    hdr = mem._header()
    return dict(params=agent.params.detach().cpu().numpy().copy(), tree=mem._grab("tree"), learns=learns,
                header=[getattr(hdr, f) for f in DS.HEADER_FIELDS], stats=env.stats(), stream_t=mem.stream_t.copy(),
                failed=mem.failed_samples(), mem=mem)


def test_train_device_on_breakout_is_deterministic_never_synchronises_and_stores_what_the_oracle_says():
    """300 rounds at S = 16 (the arguments of the Catch loop test).  Two runs end bit-identical in parameters, tree and header; a
    third under torch's sync debug mode ("error") raises nothing.  Then the oracle is replayed from the replay's own action
    column: the reward column is min(raw, 1) (reward_clip = 1, raw rewards of 2 / 3 / 4 occur), nonterminal is 0 exactly at
    the oracle's lost lives and game ends, the timestep restarts there, the frames are trunc(255 * observation)."""
    S, seed, T_max = 16, 9, 16 * 300
    a, b = _run_train(seed, T_max), _run_train(seed, T_max)
    learning_rounds = sum(1 for T in range(1, T_max + 1, S) if T >= 3200)
    assert a["learns"] == b["learns"] == learning_rounds * S // 4 and a["failed"] == 0
    assert np.array_equal(a["params"], b["params"]) and np.array_equal(a["tree"], b["tree"])
    assert a["header"] == b["header"] and a["stats"] == b["stats"] and np.array_equal(a["stream_t"], b["stream_t"])
    c = _run_train(seed, T_max, sync_debug=True)
    assert np.array_equal(a["params"], c["params"])
    mem, n = a["mem"], T_max
    col = {k: mem._grab(k, 0, n) for k in ("action", "reward", "nonterminal", "timestep", "frames")}
    ora = BO.BreakoutOracle(S, 4, 500, seed)
    stacks = ora.reset()
    t = np.zeros(S, dtype=np.int32)
    raw_above_one = life_only = overs = 0
    for r in range(T_max // S):
        rows = slice(r * S, (r + 1) * S)
        assert np.array_equal(col["frames"][rows], (stacks[:, -1] * np.float32(255)).astype(np.uint8)), r
        assert np.array_equal(col["timestep"][rows], t), r
        stacks, raw, terms = ora.step(col["action"][rows], life_terminals=True)
        assert np.array_equal(col["reward"][rows], np.minimum(raw, np.float32(1))), r
        assert np.array_equal(col["nonterminal"][rows], (~terms).astype(np.uint8)), r
        t = np.where(terms, 0, t + 1).astype(np.int32)
        raw_above_one += int((raw > 1).sum())
        life_only += sum(bool(ev["lost"] and not ev["over"]) for ev in ora.events)
        overs += sum(bool(ev["over"]) for ev in ora.events)
    assert raw_above_one >= 10 and life_only >= S and overs >= S
    assert {k: a["stats"][k] for k in BO.TOTALS} == ora.stats() and np.array_equal(a["stream_t"], t)
    assert set(np.unique(col["frames"])) == {0, 127, 191, 255}


@pytest.fixture(scope="module")
def agent(hip):
    from rainbow_amd.agent import Agent
    torch.manual_seed(3)
    np.random.seed(3)
    return Agent(_args(), types.SimpleNamespace(action_space=lambda: BO.ACTIONS))


def _oracle_evaluation(S, env_seed, episodes, actions_of):
    """test.py:19-34 on the oracle environment (evaluation mode: no life-loss terminals) with the oracle tally."""
    env, tally = BO.BreakoutOracle(S, 4, 500, env_seed), EO.TallyOracle(S, episodes)
    stacks = env.reset()
    rnd = 0
    while tally.remaining() > 0:
        stacks, rewards, terminals = env.step(actions_of(rnd, stacks), life_terminals=False)
        tally.step(rewards, ~terminals)
        rnd += 1
    returns, lengths, _ = tally.result()
    return [float(x) for x in returns], [int(x) for x in lengths]


@pytest.mark.parametrize("S,episodes", [(1, 2), (7, 10), (64, 70)])
def test_evaluate_vec_with_epsilon_one_is_the_oracle_episode_list(agent, S, episodes):
    from rainbow_amd.envs import BreakoutVec
    from rainbow_amd.loop import evaluate_vec
    env_seed, seed = 21, 5
    agent.train()
    env = BreakoutVec(S, DEV, seed=env_seed, training=False)
    out = evaluate_vec(agent, env, episodes, epsilon=1.0, seed=seed)
    assert agent.training and not env.training
    want_rewards, want_lengths = _oracle_evaluation(S, env_seed, episodes, lambda r, _: EO.eps_rows(seed, r, 0, S, 1.0, BO.ACTIONS)[1])
    assert out["rewards"] == want_rewards and len(out["rewards"]) == episodes
    assert out["lengths"] == want_lengths
    assert len(set(want_lengths)) >= min(3, episodes) and max(want_rewards) > 1.0
    assert out["avg_reward"] == sum(want_rewards) / episodes and out["Qs"] is None
    # the same call on a training-mode environment would record every life as an episode
    lives = evaluate_vec(agent, BreakoutVec(S, DEV, seed=env_seed, training=True), episodes, epsilon=1.0, seed=seed)
    assert lives["lengths"] != want_lengths


def test_evaluate_vec_with_epsilon_zero_is_the_greedy_loop(agent):
    from rainbow_amd.envs import BreakoutVec
    from rainbow_amd.loop import evaluate_vec
    S, episodes, env_seed = 7, 10, 33
    agent.eval()
    env = BreakoutVec(S, DEV, seed=env_seed)
    env.eval()
    out = evaluate_vec(agent, env, episodes, epsilon=0.0, seed=1)
    assert not agent.training
    greedy = lambda _, stacks: agent.act_batch(torch.from_numpy(stacks).to(DEV))
    want_rewards, want_lengths = _oracle_evaluation(S, env_seed, episodes, greedy)
    assert out["rewards"] == want_rewards and out["lengths"] == want_lengths


def test_state_dict_round_trip_continues_mid_game():
    """state_dict() mid-game -> load_state_dict() into a new object: the following 30 rounds are those of the object that went on."""
    from rainbow_amd.envs import BreakoutVec
    S = 7
    mk = lambda: BreakoutVec(S, DEV, seed=17, max_steps=60)
    env, ora = mk(), BO.BreakoutOracle(S, 4, 60, 17)
    env.reset(); ora.reset()
    rs = np.random.RandomState(4)
    for r in range(45):
        actions = rs.randint(0, 3, S)
        env.step_device(torch.from_numpy(actions.astype(np.int32)).to(DEV))
        ora.step(actions)
    sd = env.state_dict()
    assert min(g["t"] for g in ora.g) > 0 and sd["game"].nbytes == 64 * S and np.array_equal(sd["stacks"].numpy(), ora.stacks)
    twin = mk()
    twin.eval()
    twin.load_state_dict(sd)
    assert twin.training and twin.stats() == env.stats()
    for r in range(30):
        actions = rs.randint(0, 3, S)
        ac = torch.from_numpy(actions.astype(np.int32)).to(DEV)
        want = ora.step(actions)
        for e in (env, twin):
            st, rw, nt = e.step_device(ac)
            assert np.array_equal(st.cpu().numpy(), want[0]) and np.array_equal(rw.cpu().numpy(), want[1]), r
            assert np.array_equal(nt.cpu().numpy().astype(bool), ~want[2]), r
    assert twin.stats() == env.stats() and {k: env.stats()[k] for k in BO.TOTALS} == ora.stats()
    assert twin.state_dict()["game"].tobytes() == env.state_dict()["game"].tobytes()
    with pytest.raises(ValueError, match="max_steps"):
        BreakoutVec(S, DEV, seed=17, max_steps=61).load_state_dict(sd)
    bad = dict(sd, game=sd["game"].copy())
    bad["game"][34] = 0                                              # stream 0: lives = 0
    with pytest.raises(RuntimeError, match="rb_breakout_set_state"):
        twin.load_state_dict(bad)
    env.close(); twin.close()
