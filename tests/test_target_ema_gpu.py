"""The target network's EMA inside the optimiser pass on the MI355X: the scenarios of tests/target_ema_scenarios.py on the real
library, and the class level — an Agent with target_tau against a twin that applies the same EMA as a launch of its own, tau = 1
against a hard sync per step, and a bit-exact resume."""
import os
import types

import numpy as np
import pytest
import torch

import target_ema_scenarios as T
from rainbow_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib
    yield T.declare(_lib.load())
    out = os.environ.get("RB_OPTIMIZER_RATIOS")      # the observed error / bound table of profiles/optimizer_bounds.txt
    if out:
        with open(out, "a") as f:
            f.write(T.format_ratios("MI355X"))


@pytest.fixture
def Mem():
    from cabi_adapter import TorchMem
    return TorchMem


@pytest.mark.parametrize("n", T.PLAIN_SHAPES)
def test_rule_on_buffers_of_any_length(hip, Mem, n):
    T.plain_shapes_check(hip, Mem, n)


def test_rule_in_the_pair_workgroups_around_a_hole(hip, Mem):
    T.pair_shapes_check(hip, Mem)


def test_rule_in_every_form_of_the_small_layout(hip, Mem, monkeypatch):
    T.forms_check(hip, Mem, monkeypatch)


def test_rule_in_the_pair_pass_flushed_and_hosted(hip, Mem, monkeypatch):
    T.pairs_check(hip, Mem, monkeypatch)


def test_rule_behind_the_fused_tile_pass(hip, Mem):
    T.fused_tile_check(hip, Mem)


@pytest.mark.parametrize("flags,hows", [(L.LEARNER_DEFER_UPDATE, ("hosted", "flush")), (0, ("value",)),
                                        (L.LEARNER_FUSE_FC_H_DW | L.LEARNER_WRITE_FUSED_GRADS, ("value",))],
                         ids=["deferred", "k_clip_adam", "fused-tile"])
def test_failed_draw_leaves_the_target_alone(hip, Mem, flags, hows):
    T.failed_draw_check(hip, Mem, flags, hows)


# ---------------------------------------------------------------------------------------------------- class level --
def _args(**kw):
    base = dict(device=torch.device("cuda:0"), history_length=4, discount=0.99, multi_step=3, priority_weight=0.4,
                priority_exponent=0.5, atoms=51, V_min=-10.0, V_max=10.0, batch_size=16, norm_clip=10.0, model=None,
                learning_rate=6.25e-5, adam_eps=1.5e-4, architecture="data-efficient", hidden_size=64, noisy_std=0.1)
    base.update(kw)
    return types.SimpleNamespace(**base)


ENV = types.SimpleNamespace(action_space=lambda: 4)


def fresh(**kw):
    """The small data-efficient fixture of the class-level learner tests: the same torch seed, the same replay."""
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    args = _args(**kw)
    torch.manual_seed(77)
    np.random.seed(77)
    agent = Agent(args, ENV)
    mem = ReplayMemory(args, 2048, seed=5)
    g = torch.Generator(device="cuda").manual_seed(3)
    rs = np.random.RandomState(3)
    for _ in range(2):
        mem.append_batch(torch.randint(0, 256, (1500, 84, 84), dtype=torch.uint8, device="cuda", generator=g),
                         rs.randint(0, 4, 1500), rs.choice([-1.0, 0.0, 1.0], size=1500), rs.random_sample(1500) < 0.01)
    return agent, mem


def steps(agent, mem, ks, after=None):
    losses = []
    for k in ks:
        mem.priority_weight = min(1.0, 0.4 + 0.05 * k)
        agent.reset_noise()
        agent.learn(mem)
        losses.append(agent._loss.clone())
        if after is not None:
            after(agent)
    torch.cuda.synchronize()
    return torch.stack(losses).cpu().numpy()


def moments(agent):
    agent.flush()
    st = agent.optimiser.state[agent._params]
    return st["exp_avg"], st["exp_avg_sq"]


MODES = {"hosted": {}, "undeferred": {"RAINBOW_AMD_DEFER_UPDATE": "0"}, "stored-sigma": {"RAINBOW_AMD_IMPLICIT_SIGMA": "0"},
         "fused-dw": {"RAINBOW_AMD_FUSED_DW": "1"}, "torch-adam": {"RAINBOW_AMD_FUSED_ADAM": "0"}}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_in_pass_ema_agent_equals_twin_with_the_stand_alone_ema(hip, monkeypatch, mode):
    """Agent A: target_tau = 0.25 (the EMA rides in whatever launch carries the optimiser pass in this mode).  Agent B, same mode:
    tau = 0 and rb_learner_target_ema(0.25) after each learn().  Five steps: parameters, target parameters, the optimiser's moments
    and the five loss vectors bit-identical."""
    monkeypatch.setenv("RB_OPTS", "implicit_small=1,spec_draw=0")     # (the small net takes the (mu, sigma) pair pass only when told)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    a, ma = fresh(target_tau=0.25)
    b, mb = fresh()
    assert a.target_tau == 0.25 and b.target_tau == 0.0
    if mode == "hosted":
        assert a._defer_update and a._implicit_sigma
    if mode == "fused-dw":
        assert a._fused_dw and not a._defer_update
    t_init = a.target_params.clone()
    assert torch.equal(t_init, b.target_params)
    la = steps(a, ma, range(5))
    lb = steps(b, mb, range(5), after=lambda ag: ag.target_ema(0.25))
    if mode in ("hosted", "stored-sigma"):
        assert a._update_pending                                   # ... and target_params runs the pass
    assert np.array_equal(la, lb)
    assert torch.equal(a.params.detach(), b.params.detach())
    assert torch.equal(a.target_params, b.target_params)
    assert not a._update_pending
    assert not torch.equal(a.target_params, t_init) and not torch.equal(a.target_params, a.params.detach())
    for x, y in zip(moments(a), moments(b)):
        assert torch.equal(x, y)
    assert np.array_equal(ma._grab("tree"), mb._grab("tree"))


def test_tau_one_equals_a_hard_sync_after_every_step(hip, monkeypatch):
    monkeypatch.setenv("RB_OPTS", "implicit_small=1,spec_draw=0")
    a, ma = fresh(target_tau=1.0)
    b, mb = fresh()
    for k in range(3):
        la = steps(a, ma, [k])
        lb = steps(b, mb, [k], after=lambda ag: ag.update_target_net())
        assert np.array_equal(la, lb), k
        assert torch.equal(a.target_params, b.target_params), k
        assert torch.equal(a.target_params, a.params.detach()), k
        assert torch.equal(a.params.detach(), b.params.detach()), k


def test_update_target_net_and_the_tau_setter_keep_working(hip, monkeypatch):
    monkeypatch.setenv("RB_OPTS", "implicit_small=1,spec_draw=0")
    a, ma = fresh(target_tau=0.25)
    steps(a, ma, range(2))
    a.update_target_net()
    assert torch.equal(a.target_params, a.params.detach()) and torch.equal(a.target_noise, a.noise)
    with pytest.raises(ValueError, match="target_tau"):
        a.target_tau = 1.5
    a.target_tau = 0.0                       # off again: the next step leaves the target where the hard sync put it
    t = a.target_params.clone()
    steps(a, ma, [2])
    a.flush()
    assert torch.equal(a.target_params, t) and not torch.equal(t, a.params.detach())


def test_checkpoint_restore_resumes_bit_exactly_with_an_ema_target(hip, monkeypatch, tmp_path):
    import io
    from rainbow_amd.memory import ReplayMemory
    monkeypatch.setenv("RB_OPTS", "implicit_small=1,spec_draw=0")
    a1, m1 = fresh(target_tau=0.25)
    steps(a1, m1, range(2))
    assert a1._update_pending                # checkpoint() must run the pass before it copies the target
    ck = a1.checkpoint(str(tmp_path / "agent.ck"))
    buf = io.BytesIO()
    m1.save_to(buf, chunk_bytes=1 << 20)
    tail1 = steps(a1, m1, range(2, 4))
    a2, _unused = fresh(target_tau=0.25)
    a2.restore(str(tmp_path / "agent.ck"))
    buf.seek(0)
    m2 = ReplayMemory.load_from(buf, torch.device("cuda:0"), chunk_bytes=1 << 20)
    assert torch.equal(a2.target_params.cpu(), ck["target_params"]) and not torch.equal(ck["target_params"], ck["params"])
    tail2 = steps(a2, m2, range(2, 4))
    assert np.array_equal(tail1, tail2)
    assert torch.equal(a1.params.detach(), a2.params.detach()) and torch.equal(a1.target_params, a2.target_params)
    for x, y in zip(moments(a1), moments(a2)):
        assert torch.equal(x, y)
