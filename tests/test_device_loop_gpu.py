"""The device-resident actor loop on the MI355X: the host-interpreter checks of test_device_loop_emu.py on the device, the
Python surface (Agent.act_batch(device_out=True), CatchVec, ReplayMemory.append_streams with device operands, train_device),
a 1M-slot replay and save / restore after device rounds.  There is NO learning check here: the reference itself did not
reach the bar such a check needs on this game (tests/golden/make_golden_catch.py, profiles/catch_learning_curve.txt)."""
import io
import json
import pickle
import types

import numpy as np
import pytest
import torch

import catch_oracle as CO
import device_loop_scenarios as DS
import scenarios
from cabi_adapter import CAbiLearnAdapter, TorchMem
from oracle import learner_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib as L
    return L.load()


def _args(**kw):
    base = dict(device=torch.device("cuda:0"), history_length=4, discount=0.99, multi_step=3, priority_weight=0.4,
                priority_exponent=0.5, atoms=51, V_min=-10.0, V_max=10.0, batch_size=32, norm_clip=10.0, model=None,
                learning_rate=1e-4, adam_eps=1.5e-4, architecture="data-efficient", hidden_size=64, noisy_std=0.1,
                replay_frequency=4, target_update=500, learn_start=3200, reward_clip=1)
    base.update(kw)
    return types.SimpleNamespace(**base)


# ------------------------------------------------------------------ the emulator's checks on the device
@pytest.mark.parametrize("S", [1, 2, 7, 16, 64])
def test_device_operand_round_equals_host_operand_round_on_device(hip, S):
    DS.check_append_dev_equals_host(hip, TorchMem(), S, seed=400 + S)


def test_device_operand_round_refusals_on_device(hip):
    DS.check_append_dev_refusals(hip, TorchMem())


@pytest.mark.parametrize("history", [1, 4])
@pytest.mark.parametrize("S", [1, 7, 64])
def test_catch_kernel_matches_the_oracle_on_device(hip, S, history):
    DS.check_catch_against_oracle(hip, TorchMem(), S, history, seed=2000 * history + S)


def test_catch_seeds_and_refusals_on_device(hip):
    DS.check_catch_seeds_and_refusals(hip, TorchMem())


def test_random_policy_is_poor_on_device(hip):
    DS.check_random_policy_is_poor(hip, TorchMem())


def test_whole_device_round_equals_host_driven_round_on_device(hip):
    name = "k10"
    cfg = O.Config(**scenarios.LEARN_CONFIGS[name])

    def make_learner():
        ad = CAbiLearnAdapter(hip, TorchMem(), name)
        ad.load(O.init_params(cfg, 31), O.init_params(cfg, 32))
        ad.reset_noise_online(np.random.RandomState(6).randn(O.noise_draw_count(cfg)).astype(np.float32))
        return ad

    DS.check_device_round(hip, TorchMem(), make_learner, S=16, rounds=25)


# ------------------------------------------------------------------ the Python surface
def _same_memory(a, b, frames_rows):
    for k in ("tree", "timestep", "action", "reward", "nonterminal"):
        assert np.array_equal(a._grab(k), b._grab(k)), k
    assert np.array_equal(a._grab("frames", 0, frames_rows), b._grab("frames", 0, frames_rows))
    ha, hb = a._header(), b._header()
    assert [getattr(ha, f) for f in DS.HEADER_FIELDS] == [getattr(hb, f) for f in DS.HEADER_FIELDS]
    assert np.array_equal(a.stream_t, b.stream_t)


def test_device_rounds_at_1m_slots_equal_host_rounds():
    """A 1M-slot, 16-stream replay (the 20-level tree): 200 rounds through ReplayMemory.append_streams with device tensors
    against the same rounds with host sequences, priority write-backs in between; a third memory mixes the two."""
    from rainbow_amd.memory import ReplayMemory
    S, cap, rounds = 16, 1_000_000, 200
    host, dev = (ReplayMemory(_args(), cap, seed=3, streams=S) for _ in range(2))
    rs = np.random.RandomState(21)
    g = torch.Generator(device="cuda").manual_seed(21)
    tree_start = (1 << 20) - 1
    for r in range(rounds):
        states = torch.rand((S, 4, 84, 84), device="cuda", generator=g)
        a, rw, te = rs.randint(0, 6, S), rs.choice([-1.0, 0.0, 1.0], size=S).astype(np.float32), rs.random_sample(S) < 0.1
        host.append_streams(states, a, rw, te)
        ops = (torch.from_numpy(a.astype(np.int32)).cuda(), torch.from_numpy(rw).cuda(), torch.from_numpy(te).cuda())
        if r % 2:
            dev.append_streams(states, ops[0], ops[1], ops[2])                                      # terminals, inverted on the device
        else:
            dev.append_streams(states, ops[0], ops[1], nonterminals=(~ops[2]).to(torch.uint8))
        if r % 20 == 7:
            idx = torch.randint(0, (r + 1) * S, (64,), device="cuda", generator=g) + tree_start
            pr = torch.rand(64, device="cuda", generator=g) * 3 + 1e-3
            for m in (host, dev):
                m.update_priorities(idx, pr)
                m.flush()
        torch.cuda.synchronize()
    _same_memory(host, dev, rounds * S)
    assert host._header().index == rounds * S
    del host, dev


def test_mixed_host_and_device_rounds_equal_all_host_rounds():
    from rainbow_amd.memory import ReplayMemory
    S, cap = 8, 8 * 24
    host, mix = (ReplayMemory(_args(), cap, seed=5, streams=S) for _ in range(2))
    rs = np.random.RandomState(8)
    for r in range(80):                          # the ring wraps three times
        states = torch.from_numpy(rs.random_sample((S, 4, 84, 84)).astype(np.float32)).cuda()
        a, rw, te = rs.randint(0, 6, S), rs.choice([-1.0, 0.0, 1.0], size=S).astype(np.float32), rs.random_sample(S) < 0.2
        host.append_streams(states, a, rw, te)
        if (r // 5) % 2:
            mix.append_streams(states, torch.from_numpy(a.astype(np.int32)).cuda(), torch.from_numpy(rw).cuda(),
                               torch.from_numpy(te).cuda())
        else:
            mix.append_streams(states, a, rw, te)
        torch.cuda.synchronize()
        if r % 9 == 0:
            assert np.array_equal(host.stream_t, mix.stream_t), r
    _same_memory(host, mix, cap)


def _catch_setup(S, seed, **kw):
    from rainbow_amd.agent import Agent
    from rainbow_amd.envs import CatchVec
    from rainbow_amd.memory import ReplayMemory
    args = _args(**kw)
    torch.manual_seed(seed)
    np.random.seed(seed)
    env = CatchVec(S, args.device, seed=seed, history_length=args.history_length)
    agent = Agent(args, env)
    mem = ReplayMemory(args, kw.get("memory_capacity", 16 * 400), seed=seed, streams=S)
    return args, env, agent, mem


def _run_train(seed, T_max, sync_debug=False):
    # learn_start 3200: with S streams the sampler's last stratum must reach below the (multi_step + 1) * S newest slots, i.e.
    # more than batch_size * (multi_step + 1) * S = 2048 transitions have to be stored before the first draw can succeed
    from rainbow_amd.loop import train_device
    args, env, agent, mem = _catch_setup(16, seed)
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
    out = dict(params=agent.params.detach().cpu().numpy().copy(), tree=mem._grab("tree"), learns=learns,
               header=[getattr(hdr, f) for f in DS.HEADER_FIELDS], stats=env.stats(), stream_t=mem.stream_t.copy(),
               failed=mem.failed_samples())
    return out


def test_train_device_is_deterministic_and_never_synchronises():
    """Two runs of 300 rounds at S = 16 from the same seeds (torch, memory, environment) end with bit-identical parameters,
    replay tree and header; a third run under torch's sync debug mode ("error") raises nothing."""
    T_max = 16 * 300
    a, b = _run_train(9, T_max), _run_train(9, T_max)
    learning_rounds = sum(1 for T in range(1, T_max + 1, 16) if T >= 3200)
    assert a["learns"] == b["learns"] == learning_rounds * 16 // 4 and a["failed"] == 0
    assert np.array_equal(a["params"], b["params"]) and np.array_equal(a["tree"], b["tree"])
    assert a["header"] == b["header"] and a["stats"] == b["stats"] and np.array_equal(a["stream_t"], b["stream_t"])
    assert a["stats"]["episodes"] == 16 * (300 // 11)
    assert np.array_equal(a["stream_t"], np.full(16, 300 % 11, dtype=np.int32))
    c = _run_train(9, T_max, sync_debug=True)
    assert np.array_equal(a["params"], c["params"])
    other = _run_train(10, T_max)
    assert not np.array_equal(a["params"], other["params"])


def test_single_stream_env_surface_matches_the_oracle():
    """CatchVec(streams=1) through the reference's Env surface (reset / step(int) / reset after done) against CatchEnv."""
    from rainbow_amd.envs import CatchVec
    env, ora = CatchVec(1, "cuda:0", seed=44), CO.CatchEnv(44)
    rs = np.random.RandomState(2)
    assert env.action_space() == ora.action_space() == 3
    done = True
    for t in range(40):
        if done:
            s, so = env.reset(), ora.reset()
            assert np.array_equal(s.cpu().numpy(), so.numpy())
        a = int(rs.randint(0, 3))
        (s, r, done), (so, ro, do) = env.step(a), ora.step(a)
        assert (r, done) == (ro, do) and np.array_equal(s.cpu().numpy(), so.numpy()), t
    assert env.stats()["episodes"] == 3
    env.close()


def test_save_and_pickle_after_device_rounds_keep_stream_timesteps():
    from rainbow_amd.memory import ReplayMemory
    S = 7
    args, env, agent, mem = _catch_setup(S, 12, memory_capacity=7 * 64)
    ora = CO.CatchOracle(S, 4, 12)
    stacks = env.reset()
    ora.reset()
    t = np.zeros(S, dtype=np.int32)
    rs = np.random.RandomState(3)
    for r in range(22):
        if r == 13:                               # from here on the streams' counters are out of step with each other
            stacks = env.reset(); ora.reset()
            mem.append_streams(stacks, torch.zeros(S, dtype=torch.int32, device="cuda"), torch.zeros(S, device="cuda"),
                               torch.from_numpy(np.arange(S) % 2 == 0).cuda())
            t = np.where(np.arange(S) % 2 == 0, 0, t + 1).astype(np.int32)
        actions = torch.from_numpy(rs.randint(0, 3, S).astype(np.int32)).cuda()
        nxt, rewards, terminals = env.step(actions)
        _, _, want_term = ora.step(actions.cpu().numpy())
        mem.append_streams(stacks, actions, rewards, terminals)
        t = np.where(want_term, 0, t + 1).astype(np.int32)
        stacks = nxt
    buf = io.BytesIO()
    mem.save_to(buf)
    meta_len = int.from_bytes(buf.getvalue()[8:16], "little")
    assert json.loads(buf.getvalue()[16:16 + meta_len].decode())["stream_t"] == [int(x) for x in t]
    assert len(set(int(x) for x in t)) == 2
    buf.seek(0)
    back = ReplayMemory.load_from(buf, "cuda:0")
    assert np.array_equal(back.stream_t, t) and np.array_equal(mem.stream_t, t)
    # device rounds again (the counters go back to the device), then a pickle
    actions = torch.zeros(S, dtype=torch.int32, device="cuda")
    nxt, rewards, terminals = env.step(actions)
    _, _, want_term = ora.step(np.zeros(S, dtype=np.int64))
    mem.append_streams(stacks, actions, rewards, terminals)
    t = np.where(want_term, 0, t + 1).astype(np.int32)
    clone = pickle.loads(pickle.dumps(mem))
    assert np.array_equal(clone.stream_t, t) and np.array_equal(mem.stream_t, t)
    assert np.array_equal(clone._grab("timestep"), mem._grab("timestep"))
    clone.append_streams(nxt, actions, rewards, terminals)          # and the restored memory goes on with device rounds
    torch.cuda.synchronize()
    assert np.array_equal(clone.stream_t, np.where(want_term, 0, t + 1))
