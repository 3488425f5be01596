"""Device-side diagnostics on the MI355X: the bodies of diag_scenarios.py through the C ABI (every case of the host-interpreter
run, plus the canonical net at batch 32 — more norm partials than the 256 threads that sum them — and a replay of 2^20 slots),
and the Python layer on top: Agent.track_stats / read_stats, Agent.evaluate_loss, ReplayMemory.priority_stats."""
import types

import numpy as np
import pytest
import torch

import diag_scenarios as DS
from cabi_adapter import TorchMem

pytestmark = pytest.mark.gpu

ALL_CASES = sorted(DS.CASES) + sorted(DS.GPU_ONLY_CASES)


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", ALL_CASES)
def test_step_records_eager_path_on_device(hip, case):
    DS.check_records_eager(hip, TorchMem(), case)


@pytest.mark.parametrize("case", ALL_CASES)
def test_step_records_one_call_path_on_device(hip, case):
    DS.check_records_one_call(hip, TorchMem(), case)


def test_ring_wraps_on_device(hip):
    DS.check_ring_wraps(hip, TorchMem())


def test_failed_draw_is_recorded_and_does_not_advance_the_step_on_device(hip):
    DS.check_failed_draw(hip, TorchMem())


def test_exchange_leaves_no_norm_and_blocks_eval_loss_on_device(hip):
    DS.check_exchange_gives_nan(hip, TorchMem())


def test_records_are_deterministic_and_the_off_switch_changes_nothing_on_device(hip):
    DS.check_deterministic_and_off(hip, TorchMem(), count_launches=True)


@pytest.mark.parametrize("case", ALL_CASES)
def test_eval_loss_matches_the_oracle_on_device(hip, case):
    DS.check_eval_loss(hip, TorchMem(), case)


def test_eval_loss_has_no_side_effects_on_device(hip):
    DS.check_eval_no_side_effects(hip, TorchMem())


def test_eval_loss_and_set_stats_refuse_bad_arguments_on_device(hip):
    DS.check_eval_refusals(hip, TorchMem())


@pytest.mark.parametrize("state", DS.PSTATS_STATES)
@pytest.mark.parametrize("capacity", DS.PSTATS_CAPACITIES + [1 << 20])
def test_priority_stats_on_device(hip, capacity, state):
    DS.check_priority_stats(hip, TorchMem(), capacity, state)


def test_priority_stats_refuses_null_on_device(hip):
    DS.check_priority_stats_refusals(hip, TorchMem())


# =============================================================================== the Python layer
def _args(**kw):
    base = dict(device=torch.device("cuda:0"), history_length=4, discount=0.99, multi_step=3, priority_weight=0.4,
                priority_exponent=0.5, atoms=51, V_min=-10.0, V_max=10.0, batch_size=6, norm_clip=10.0, model=None,
                learning_rate=6.25e-5, adam_eps=1.5e-4, architecture="data-efficient", hidden_size=32, noisy_std=0.1)
    base.update(kw)
    return types.SimpleNamespace(**base)


ENV = types.SimpleNamespace(action_space=lambda: 4)


def _filled_memory(args, capacity=512, appends=400, seed=11):
    from rainbow_amd.memory import ReplayMemory
    mem = ReplayMemory(args, capacity, seed=seed)
    rs = np.random.RandomState(seed)
    for _ in range(appends):
        st = torch.from_numpy(rs.randint(0, 256, size=(4, 84, 84)).astype(np.float32) / np.float32(255)).cuda()
        mem.append(st, int(rs.randint(0, 4)), float(rs.choice([-1.0, 0.0, 1.0])), bool(rs.random_sample() < 0.05))
    return mem


def test_agent_read_stats_returns_the_records_in_order_and_counts_the_dropped(hip):
    """args.step_stats = 3 and five learn steps: read_stats() hands back steps 3, 4, 5 and dropped = 2; two more steps, then the
    next read returns exactly those two and dropped = 0; loss_mean is the mean of the agent's own loss buffer, grad_norm the bits
    of its norm; track_stats(0) switches the records off and read_stats() returns None."""
    from rainbow_amd.agent import Agent
    torch.manual_seed(5)
    args = _args(step_stats=3)
    agent = Agent(args, ENV)
    mem = _filled_memory(args)
    for _ in range(5):
        agent.learn(mem)
    r = agent.read_stats()
    assert r["dropped"] == 2 and r["step"].tolist() == [3, 4, 5] and r["batch"].tolist() == [6] * 3 and r["status"].tolist() == [0] * 3
    assert set(r) == set(DS.STEP_STATS_DTYPE.names) - {"reserved"} | {"dropped"}
    np.testing.assert_allclose(r["loss_mean"][-1], agent._loss.double().mean().item(), rtol=1e-6)
    assert np.float32(r["grad_norm"][-1]).view(np.uint32) == agent._norm.cpu().numpy().view(np.uint32)[0]      # (_norm flushes)
    for _ in range(2):
        agent.learn(mem)
    r = agent.read_stats()
    assert r["dropped"] == 0 and r["step"].tolist() == [6, 7]
    r = agent.read_stats()
    assert r["dropped"] == 0 and r["step"].size == 0
    agent.track_stats(0)
    agent.learn(mem)
    assert agent.read_stats() is None
    # an agent that never asked for records has none
    assert Agent(_args(), ENV).read_stats() is None


def test_agent_evaluate_loss_is_repeatable_and_leaves_the_memory_priorities_alone(hip):
    """Agent.evaluate_loss on a validation memory with injected uniforms: the same numbers twice, no priority changed, the
    agent's parameters untouched; a horizon mismatch raises the ValueError of learn()."""
    from rainbow_amd.agent import Agent
    torch.manual_seed(6)
    args = _args()
    agent = Agent(args, ENV)
    mem, val = _filled_memory(args), _filled_memory(args, seed=12)
    for _ in range(2):
        agent.learn(mem)
    uu = torch.from_numpy(np.random.RandomState(3).random_sample((32, 6))).cuda()
    params = agent.params.detach().clone()
    tree = val.priority_stats()
    a = agent.evaluate_loss(val, batches=2, unit_uniforms=uu)
    b = agent.evaluate_loss(val, batches=2, unit_uniforms=uu)
    assert a["loss"].shape == (2, 6) and np.isfinite(a["loss"]).all() and a["batches"] == 2
    assert np.array_equal(a["loss"].view(np.uint32), b["loss"].view(np.uint32))
    assert {k: v for k, v in a.items() if k != "loss"} == {k: v for k, v in b.items() if k != "loss"}
    np.testing.assert_allclose(a["loss_mean"], a["loss"].astype(np.float64).mean(), rtol=1e-6)
    assert a["weight_mean"] == 1.0 and a["loss_max"] == float(a["loss"].max())
    after = val.priority_stats()
    assert {k: (v.tolist() if k == "hist" else v) for k, v in tree.items()} == {k: (v.tolist() if k == "hist" else v) for k, v in after.items()}
    assert torch.equal(params, agent.params.detach())
    from rainbow_amd import loop
    res = loop._evaluation_result(agent, [1.0], [1], val, with_loss=True)
    assert np.isfinite(res["val_loss"]) and np.isfinite(res["val_td_abs"]) and "val_loss" not in loop._evaluation_result(agent, [1.0], [1], val)
    val.set_horizon(2)
    with pytest.raises(ValueError, match="horizon"):
        agent.evaluate_loss(val)


def test_agent_evaluate_loss_raises_when_the_draw_finds_no_batch(hip):
    """A validation memory too small for the batch (16 slots, the write head's exclusion zone covers stratum 0): the sampler gives up,
    the stacks are stale, and evaluate_loss says so instead of returning their loss; the counter is cleared for the next caller."""
    from rainbow_amd.agent import Agent
    args = _args()
    agent = Agent(args, ENV)
    tiny = _filled_memory(args, capacity=16, appends=16)
    with pytest.raises(RuntimeError, match="no valid batch"):
        agent.evaluate_loss(tiny)
    assert tiny.failed_samples() == 0


def test_memory_priority_stats_applies_a_pending_update_first(hip):
    """ReplayMemory.priority_stats: ess, hist and hist_lo_exp beside the raw fields, against numpy on the leaves; a lazy
    update_priorities() recorded before the call is in the numbers."""
    args = _args()
    mem = _filled_memory(args, capacity=256, appends=200)
    o = mem.sample_device(6)
    idx = o["tree_idxs"].clone()
    mem.update_priorities(idx, torch.full((6,), 4.0, device="cuda"))           # lazy: rides in the next draw — or is applied here
    s = mem.priority_stats()
    import ctypes as C
    from rainbow_amd import _lib as L
    b = L.ReplayBuffers()
    L.check(hip, hip.rb_replay_buffers(mem._h, C.byref(b)))
    tree = TorchMem().view(b.sum_tree_dev, (b.tree_len,), np.float32)
    want = DS.pstats_reference(tree[b.tree_start:b.tree_start + 256])
    assert s["max"] == np.float32(4.0 ** 0.5) == want["max"], (s["max"], want["max"])
    assert (s["nonzero"], s["invalid"], s["min_pos"]) == (want["nonzero"], want["invalid"], float(want["min_pos"]))
    assert np.array_equal(s["hist"], want["hist"]) and s["hist_lo_exp"] == -40
    np.testing.assert_allclose([s["sum"], s["sumsq"], s["ess"]], [want["sum"], want["sumsq"], want["sum"] ** 2 / want["sumsq"]], rtol=1e-9)
    assert 1.0 <= s["ess"] <= s["nonzero"]
