"""The annealed update horizon and discount on the MI355X: every row of tests/horizon_scenarios.py against librainbow_hip.so
(rb_replay_set_horizon, k_set_horizon, the sampler and the two gathers at n_eff of n_max; rb_learner_set_horizon), then the drop-in
classes — ReplayMemory.set_horizon / Agent.set_horizon, Agent.learn on the zero-copy path under a changing horizon against the oracle
replay and the oracle learner, and the saved state (save_to / load_from, pickling, Agent.checkpoint) at horizon 3 of 10."""
import copy
import io
import json
import pickle
import struct
import types

import numpy as np
import pytest
import torch

import horizon_scenarios as HZ
from cabi_adapter import TorchMem
from guarded_mem import GuardedTorchMem
from oracle import learner_oracle as O
from oracle.replay_oracle import ReplayOracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib as L
    return L.load()


# =============================================================================== A. replay
@pytest.mark.parametrize("row", HZ.A1_ROWS, ids=HZ.a1_id)
def test_batch_at_n_eff_is_the_oracle_built_with_n_eff_on_device(hip, row):
    HZ.check_table_row(hip, TorchMem(), row)


def test_episode_ends_inside_at_and_beyond_the_horizon_on_device(hip):
    HZ.check_episode_ends(hip, TorchMem())


@pytest.mark.parametrize("streams,cap", [(1, 96), (3, 192)], ids=["S1", "S3"])
def test_write_head_rule_follows_the_horizon_on_device(hip, streams, cap):
    HZ.check_write_head(hip, GuardedTorchMem(), S=streams, cap=cap)


def test_rejection_loop_and_weights_under_random_priorities_on_device(hip):
    HZ.check_random_priorities(hip, TorchMem())


def test_horizon_changes_on_a_live_replay_on_device(hip):
    HZ.check_live_change(hip, TorchMem())


def test_refusals_name_the_argument_and_leave_the_replay_working_on_device(hip):
    HZ.check_refusals(hip, TorchMem())


# =============================================================================== B. learner
def test_learner_refusals_on_device(hip):
    HZ.check_learner_refusals(hip, TorchMem())


@pytest.mark.parametrize("row", sorted(HZ.LEARN_ROWS))
def test_two_learn_steps_under_two_horizons_match_the_oracle_on_device(hip, row):
    """The gathered path (rb_learner_learn) at the data-efficient batch-4 row and at the canonical net, batch 32, hidden 512."""
    HZ.check_learn(hip, TorchMem(), row)


def test_train_step_refuses_mismatched_horizons_on_device(hip):
    HZ.check_train_step_mismatch(hip, TorchMem)


def test_train_step_follows_the_horizon_on_device(hip, monkeypatch):
    HZ.check_train_step(hip, TorchMem, monkeypatch, spec=False)


def test_early_draw_made_under_the_old_horizon_is_discarded_on_device(hip, monkeypatch):
    HZ.check_train_step(hip, TorchMem, monkeypatch, spec=True)


# =============================================================================== the classes
def _args(**kw):
    base = dict(device=torch.device("cuda:0"), history_length=4, discount=HZ.G0, multi_step=10, priority_weight=0.4,
                priority_exponent=0.5, atoms=51, V_min=-10.0, V_max=10.0, batch_size=4, norm_clip=10.0, model=None,
                learning_rate=6.25e-5, adam_eps=1.5e-4, architecture="data-efficient", hidden_size=32, noisy_std=0.1, seed=3)
    base.update(kw)
    return types.SimpleNamespace(**base)


ENV = types.SimpleNamespace(action_space=lambda: 6)


def _filled(args, cap, total, seed, horizons=()):
    """A ReplayMemory and one ReplayOracle per (n, gamma), all fed the same `total` transitions."""
    from rainbow_amd.memory import ReplayMemory
    mem = ReplayMemory(args, cap, seed=seed)
    oras = {hz: ReplayOracle(cap, history=4, discount=hz[1], multi_step=hz[0]) for hz in horizons}
    rs = np.random.RandomState(seed)
    rows = HZ.make_rows(total, 1, rs, p_term=0.04)
    terminals = rows["nt"] == 0
    for lo in range(0, total, cap // 2):
        sl = slice(lo, min(total, lo + cap // 2))
        frames = rows["pool"][(np.arange(sl.start, sl.stop) * 7) % 64]
        mem.append_batch(torch.from_numpy(frames).cuda(), rows["actions"][sl], rows["rewards"][sl], terminals[sl])
        for ora in oras.values():
            ora.transitions.bulk_append(rows["ts"][sl], frames, rows["actions"][sl], rows["rewards"][sl], ~terminals[sl])
    return mem, oras


def test_agent_learn_on_the_zero_copy_path_follows_the_horizon(hip):
    """Agent.learn(mem) end to end at the canonical net, batch 32, hidden 512 (conv1 reads the ring through the window table: slot
    n_eff + c of a row whose stride stays history + 10): agent and memory created with multi_step 10, set to (3, 0.997) before step
    0 and (7, 0.98) before step 1, against the oracle replay built with that n and the oracle learner configured with the same
    (n, gamma) — the comparison of test_agent_and_memory_classes_end_to_end_vs_oracle, its tolerances unchanged."""
    from rainbow_amd.agent import Agent
    args = _args(architecture="canonical", hidden_size=512, batch_size=32)
    B, cap = 32, 4096
    torch.manual_seed(3)
    agent = Agent(args, ENV)
    mem, oras = _filled(args, cap, 6000, 11, HZ.HORIZON_STEPS)
    assert (agent.n, agent.horizon, agent.discount, mem.n, mem.horizon, mem.discount) == (10, 10, HZ.G0, 10, 10, HZ.G0)
    online = {k: v.cpu().numpy() for k, v in agent.state_dict().items() if "epsilon" not in k}
    target = {k: v.copy() for k, v in online.items()}
    adam = O.AdamOracle(online, args.learning_rate, args.adam_eps)
    rs = np.random.RandomState(21)
    for step, (n, g) in enumerate(HZ.HORIZON_STEPS):
        agent.set_horizon(n, g)
        mem.set_horizon(n, g)
        assert (agent.horizon, agent.discount, mem.horizon, mem.discount, agent.n, mem.n) == (n, g, n, g, 10, 10)
        cfg = O.Config(batch=B, atoms=51, actions=6, history=4, hidden=512, architecture="canonical", multi_step=n, discount=g)
        draws = O.noise_draw_count(cfg)
        raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
        uu = rs.random_sample((32, B))
        agent.reset_noise(torch.from_numpy(raw_on))
        agent.learn(mem, _target_raw_normals=torch.from_numpy(raw_tg), _unit_uniforms=torch.from_numpy(uu))
        assert agent._zero_copy_ok, "the row is about the zero-copy path"
        ora = oras[(n, g)]
        ora.priority_weight = mem.priority_weight
        batch = ora.sample_with_uniforms(B, uu)
        want = O.learn(cfg, online, target, O.make_noise(cfg, raw_on), O.make_noise(cfg, raw_tg), batch)
        total, clipped = O.clip_grads(want["grads"], args.norm_clip)
        online = adam.step(clipped)
        for o in oras.values():
            o.update_priorities(batch["tree_idxs"], want["loss"])
        torch.cuda.synchronize()
        out = mem._out[B]
        assert np.array_equal(out["tree_idxs"].cpu().numpy(), batch["tree_idxs"]), "step %d" % step
        assert np.array_equal(out["returns"].cpu().numpy().view(np.uint32), batch["returns"].view(np.uint32)), "step %d" % step
        assert np.array_equal(out["nonterminals"].cpu().numpy(), batch["nonterminals"][:, 0]), "step %d" % step
        np.testing.assert_allclose(agent._loss.cpu().numpy(), want["loss"], rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(float(agent._norm.item()), total, rtol=2e-5)
        got = {k: v.cpu().numpy() for k, v in agent.state_dict().items() if "epsilon" not in k}
        for k in online:
            np.testing.assert_allclose(got[k], online[k], rtol=0, atol=3e-7, err_msg="step %d %s" % (step, k))


def test_agent_learn_raises_on_mismatched_horizons(hip):
    """The memory at 3, the agent at 10 (then the horizons equal and the discounts not): ValueError from a host compare, before
    anything is launched — the replay's header (its RNG counter and attempt count included) and the loss buffer keep their bytes."""
    from rainbow_amd.agent import Agent
    args = _args()
    agent = Agent(args, ENV)
    mem, _ = _filled(args, 512, 700, 5)
    agent.learn(mem)
    agent.flush()
    torch.cuda.synchronize()
    hdr0, loss0, params0 = bytes(mem._header()), agent._loss.clone(), agent.params.detach().clone()
    mem.set_horizon(3, HZ.GAMMA)
    with pytest.raises(ValueError, match="horizon"):
        agent.learn(mem)
    agent.set_horizon(3)                                   # (None keeps the agent's discount: still 0.97 against 0.997)
    assert (agent.horizon, agent.discount) == (3, HZ.G0)
    with pytest.raises(ValueError, match="discount"):
        agent.learn(mem)
    torch.cuda.synchronize()
    assert bytes(mem._header()) == hdr0 and torch.equal(agent._loss, loss0) and torch.equal(agent.params.detach(), params0)
    agent.set_horizon(3, HZ.GAMMA)
    agent.learn(mem)
    torch.cuda.synchronize()
    assert mem.failed_samples() == 0 and bytes(mem._header()) != hdr0
    for obj in (agent, mem):
        for n, g in ((0, None), (11, None), (3, 0.0), (3, 1.5)):
            with pytest.raises(ValueError):
                obj.set_horizon(n, g)
        assert (obj.horizon, obj.discount, obj.n) == (3, HZ.GAMMA, 10)


def _strip_stream_meta(blob, keys):
    """A save_to stream with `keys` removed from its metadata: what a file written before they existed looks like."""
    assert blob[:8] == b"RBRPLY01"
    (n,) = struct.unpack("<q", blob[8:16])
    meta = json.loads(blob[16:16 + n].decode())
    for k in keys:
        del meta[k]
    head = json.dumps(meta).encode()
    return b"RBRPLY01" + struct.pack("<q", len(head)) + head + blob[16 + n:]


def test_saved_state_carries_the_horizon(hip):
    """save_to / load_from, pickling and Agent.checkpoint() at horizon 3 of 10: after one learn step the pair is saved three ways;
    each restored pair then draws and learns bit-identically to the original for two more steps (batch indices, returns, loss,
    parameters, the replay's tree).  State written before the horizon existed — the stream's metadata, the pickle's dict and the
    checkpoint without the new keys — restores at horizon == n."""
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    args = _args()
    B = args.batch_size
    torch.manual_seed(5)
    agent = Agent(args, ENV)
    mem, _ = _filled(args, 512, 700, 9)
    for obj in (agent, mem):
        obj.set_horizon(3, HZ.GAMMA)
    agent.learn(mem)
    ck = copy.deepcopy(agent.checkpoint())
    assert (ck["horizon"], ck["discount"]) == (3, HZ.GAMMA)
    pickled = pickle.dumps(mem)
    buf = io.BytesIO()
    mem.save_to(buf)
    restored = []
    for how in ("pickle", "stream"):
        m2 = pickle.loads(pickled) if how == "pickle" else ReplayMemory.load_from(io.BytesIO(buf.getvalue()), args.device)
        assert (m2.horizon, m2.discount, m2.n) == (3, HZ.GAMMA, 10), how
        a2 = Agent(args, ENV)
        assert (a2.horizon, a2.discount) == (10, HZ.G0)
        a2.restore(copy.deepcopy(ck))
        assert (a2.horizon, a2.discount, a2.n) == (3, HZ.GAMMA, 10), how
        restored.append((how, a2, m2))
    for step in range(2):
        agent.learn(mem)
        torch.cuda.synchronize()
        want = dict(idx=mem._out[B]["tree_idxs"].cpu(), ret=mem._out[B]["returns"].cpu(), loss=agent._loss.cpu().clone(),
                    params=agent.params.detach().cpu().clone(), tree=mem._dump()["tree"].copy())
        for how, a2, m2 in restored:
            a2.learn(m2)
            torch.cuda.synchronize()
            assert torch.equal(m2._out[B]["tree_idxs"].cpu(), want["idx"]), (how, step)
            assert torch.equal(m2._out[B]["returns"].cpu(), want["ret"]), (how, step)
            assert torch.equal(a2._loss.cpu(), want["loss"]), (how, step)
            assert torch.equal(a2.params.detach().cpu(), want["params"]), (how, step)
            assert np.array_equal(m2._dump()["tree"], want["tree"]), (how, step)
    # ---- state from before the horizon existed
    old = ReplayMemory.load_from(io.BytesIO(_strip_stream_meta(buf.getvalue(), ["horizon"])), args.device)
    assert (old.horizon, old.n) == (10, 10)
    st = mem.__getstate__()
    del st["horizon"]
    old = ReplayMemory.__new__(ReplayMemory)
    old.__setstate__(st)
    assert (old.horizon, old.n) == (10, 10)
    old_ck = {k: v for k, v in ck.items() if k not in ("horizon", "discount")}
    a3 = Agent(args, ENV)
    a3.set_horizon(5, 0.98)
    a3.restore(old_ck)
    assert (a3.horizon, a3.discount) == (10, HZ.G0)
