"""Shrink-and-perturb resets on the MI355X: the scenarios of tests/reset_scenarios.py on the real library, bit for bit against
tests/reset_oracle.py, and the class level — Agent.reset_parameters against a pending optimiser pass, against the oracle's result
written by hand, with a restarted Adam step, under an EMA target, and across checkpoint() / restore()."""
import types

import numpy as np
import pytest
import torch

import optimizer_scenarios as S
import reset_oracle as RO
import reset_scenarios as R

pytestmark = pytest.mark.gpu

NETS = sorted(R.NETS)


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib
    return _lib.load()


@pytest.fixture
def Mem():
    from cabi_adapter import TorchMem
    return TorchMem


# ----------------------------------------------------------------------------------------------------- kernel level --
@pytest.mark.parametrize("net", NETS)
def test_result_equals_the_oracle_bit_for_bit(hip, Mem, net):
    R.oracle_check(hip, Mem, net)


@pytest.mark.parametrize("net", NETS)
def test_full_reset_does_not_read_non_finite_parameters(hip, Mem, net):
    R.bad_inputs_check(hip, Mem, net)


@pytest.mark.parametrize("net", NETS)
def test_target_and_moments_can_be_left_out(hip, Mem, net):
    R.target_off_check(hip, Mem, net)


@pytest.mark.parametrize("net", NETS)
def test_draw_is_keyed_by_seed_and_draw_only(hip, Mem, net):
    R.keys_check(hip, Mem, net)


@pytest.mark.parametrize("net", NETS)
def test_largest_tensor_is_uniform_inside_its_bound(hip, Mem, net):
    R.distribution_check(hip, Mem, net)


def test_alpha_outside_the_unit_interval_is_refused_by_name(hip, Mem):
    R.invalid_args_check(hip, Mem)


# ---------------------------------------------------------------------------------------------------- class level --
# (the fixture of tests/test_target_ema_gpu.py: data-efficient, hidden 64, batch 16, replay 2048)
def _args(**kw):
    base = dict(device=torch.device("cuda:0"), history_length=4, discount=0.99, multi_step=3, priority_weight=0.4,
                priority_exponent=0.5, atoms=51, V_min=-10.0, V_max=10.0, batch_size=16, norm_clip=10.0, model=None,
                learning_rate=6.25e-5, adam_eps=1.5e-4, architecture="data-efficient", hidden_size=64, noisy_std=0.1)
    base.update(kw)
    return types.SimpleNamespace(**base)


ENV = types.SimpleNamespace(action_space=lambda: 4)


def fresh(**kw):
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


def steps(agent, mem, ks):
    losses = []
    for k in ks:
        mem.priority_weight = min(1.0, 0.4 + 0.05 * k)
        agent.reset_noise()
        agent.learn(mem)
        losses.append(agent._loss.clone())
    torch.cuda.synchronize()
    return torch.stack(losses).cpu().numpy()


def moments(agent):
    agent.flush()
    st = agent.optimiser.state[agent._params]
    return st["exp_avg"], st["exp_avg_sq"]


def snapshot(agent):
    """p, t, m, v as numpy (a pending pass runs first)."""
    m, v = moments(agent)
    torch.cuda.synchronize()
    return dict(p=agent.params.detach().cpu().numpy().copy(), t=agent.target_params.cpu().numpy().copy(),
                m=m.cpu().numpy().copy(), v=v.cpu().numpy().copy())


def layout_of(agent):
    return {name: (off, shape) for name, off, shape in agent._layout}


def same_agents(a, b, label):
    sa, sb = snapshot(a), snapshot(b)
    for k in "ptmv":
        assert np.array_equal(R._bits(sa[k]), R._bits(sb[k])), (label, k)


MODES = {"hosted": {}, "undeferred": {"RAINBOW_AMD_DEFER_UPDATE": "0"}, "torch-adam": {"RAINBOW_AMD_FUSED_ADAM": "0"}}
AE, AH, RNG = 0.5, 0.0, (9, 2 ** 32 + 1)


def _mode(monkeypatch, mode):
    monkeypatch.setenv("RB_OPTS", "implicit_small=1,spec_draw=0")     # (the small net takes the (mu, sigma) pair pass only when told)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


def head_mask(agent):
    mask = np.zeros(agent._params.numel(), bool)
    for name, (off, numel, _u, _v, enc) in RO.tensor_rules(layout_of(agent), 0.1).items():
        mask[off:off + numel] = not enc
    return mask


@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_pending_pass_runs_before_the_reset(hip, monkeypatch, mode):
    """A: two learn(), then reset_parameters() while the second step's pass is still pending.  B: two learn(), flush(), then the
    reset.  Parameters, target and moments bit-identical, and equal to the oracle's result from B's flushed state: the alpha = 0
    tensors are phi exactly (phi plus an Adam step had the pass run late)."""
    _mode(monkeypatch, mode)
    a, ma = fresh()
    b, mb = fresh()
    steps(a, ma, range(2))
    steps(b, mb, range(2))
    if mode == "hosted":
        assert a._defer_update and a._update_pending
    a.reset_parameters(AE, AH, rng=RNG)
    assert not a._update_pending and a.resets == 1
    b.flush()
    st = snapshot(b)
    b.reset_parameters(AE, AH, rng=RNG)
    same_agents(a, b, mode)
    want, touched = RO.shrink_perturb(layout_of(b), st, AE, AH, 0.1, *RNG)
    phi, _ = RO.phi_flat(layout_of(b), st["p"].size, 0.1, *RNG)
    head = head_mask(b)
    assert head.any() and touched.any()
    for ag in (a, b):
        got = snapshot(ag)
        for k in "ptmv":
            assert np.array_equal(R._bits(got[k]), R._bits(want[k])), (mode, k)
        assert np.array_equal(R._bits(got["p"][head]), R._bits(phi[head])) and np.array_equal(R._bits(got["t"][head]), R._bits(phi[head]))
    with pytest.raises(ValueError, match="shrink_encoder"):
        a.reset_parameters(1.5, 0.0)
    with pytest.raises(ValueError, match="shrink_head"):
        a.reset_parameters(0.5, float("nan"))
    assert a.resets == 1


@pytest.mark.parametrize("mode", sorted(MODES))
def test_reset_leaves_no_hidden_state(hip, monkeypatch, mode):
    """A resets through the library.  B gets the oracle's result written by hand through torch (params, target_params, zeroed
    moments).  Two further learn() calls on each: loss vectors, parameters, target, moments and the replay tree bit-identical."""
    _mode(monkeypatch, mode)
    a, ma = fresh()
    b, mb = fresh()
    steps(a, ma, range(2))
    steps(b, mb, range(2))
    a.reset_parameters(AE, AH, rng=RNG)
    want, _ = RO.shrink_perturb(layout_of(b), snapshot(b), AE, AH, 0.1, *RNG)
    mb_, vb_ = moments(b)
    with torch.no_grad():
        b.params.detach().copy_(torch.from_numpy(want["p"]))
        b.target_params.copy_(torch.from_numpy(want["t"]))
        mb_.copy_(torch.from_numpy(want["m"]))
        vb_.copy_(torch.from_numpy(want["v"]))
    same_agents(a, b, (mode, "right after the reset"))
    la, lb = steps(a, ma, range(2, 4)), steps(b, mb, range(2, 4))
    assert np.array_equal(la, lb)
    same_agents(a, b, (mode, "two steps later"))
    assert np.array_equal(ma._grab("tree"), mb._grab("tree"))


@pytest.mark.parametrize("mode", ["hosted", "undeferred"])
def test_restart_step_makes_the_next_update_a_first_adam_step(hip, monkeypatch, mode):
    """restart_step=True: the step after the reset is held to the float64 one-step Adam reference AT STEP 1 with the bounds of
    tests/optimizer_scenarios.py (check_update), from the device's own state and stored (clipped) gradient.  Without it the step
    number goes on counting."""
    _mode(monkeypatch, mode)
    a, ma = fresh()
    steps(a, ma, range(2))
    a.reset_parameters(AE, AH, rng=RNG)
    a._sync_step()
    assert float(a.optimiser.state[a._params]["step"]) == 2.0           # the default leaves the step alone
    a.reset_parameters(AE, AH, rng=(9, 7), restart_step=True)
    assert float(a.optimiser.state[a._params]["step"]) == 0.0
    if a._step_dev is not None:
        assert int(a._step_dev.item()) == 0
    before = snapshot(a)
    assert not before["m"][head_mask(a)].any()
    steps(a, ma, [2])
    gp = a.grads.detach().cpu().numpy().copy()
    after = snapshot(a)
    a._sync_step()
    assert float(a.optimiser.state[a._params]["step"]) == 1.0
    assert not np.array_equal(after["p"], before["p"])
    S.check_update("reset_" + mode, before, after, gp, 1, "restart_step / " + mode)


def test_restart_step_reaches_torch_own_adam(hip, monkeypatch):
    """RAINBOW_AMD_FUSED_ADAM=0: the moments cleared and the step restarted are those of torch's optimiser.  Twin B gets the same
    reset and has its state's step zeroed by hand; the next learn() is bit-identical."""
    _mode(monkeypatch, "torch-adam")
    a, ma = fresh()
    b, mb = fresh()
    steps(a, ma, range(2))
    steps(b, mb, range(2))
    a.reset_parameters(AE, AH, rng=RNG, restart_step=True)
    b.reset_parameters(AE, AH, rng=RNG)
    assert float(a.optimiser.state[a._params]["step"]) == 0.0 and float(b.optimiser.state[b._params]["step"]) == 2.0
    assert not moments(a)[0][torch.from_numpy(head_mask(a)).to(a.device)].any()
    b.optimiser.state[b._params]["step"].zero_()
    la, lb = steps(a, ma, [2]), steps(b, mb, [2])
    assert np.array_equal(la, lb)
    same_agents(a, b, "torch-adam, restarted")
    assert float(a.optimiser.state[a._params]["step"]) == 1.0


@pytest.mark.parametrize("mode", sorted(MODES))
def test_target_equals_online_after_a_reset_with_tau_one(hip, monkeypatch, mode):
    _mode(monkeypatch, mode)
    a, ma = fresh(target_tau=1.0)
    steps(a, ma, range(2))
    t_before = a.target_params.clone()
    a.reset_parameters(AE, AH, rng=RNG)
    assert torch.equal(a.target_params, a.params.detach()) and not torch.equal(a.target_params, t_before)
    steps(a, ma, [2])
    assert torch.equal(a.target_params, a.params.detach())


def test_checkpoint_restore_resumes_bit_exactly_across_resets(hip, monkeypatch, tmp_path):
    import io
    from rainbow_amd.memory import ReplayMemory
    _mode(monkeypatch, "hosted")
    a1, m1 = fresh()
    steps(a1, m1, range(2))
    a1.reset_parameters()                              # reset #1: the defaults, rng = (args.seed or 0, 0)
    assert a1.resets == 1
    ck = a1.checkpoint(str(tmp_path / "agent.ck"))
    assert ck["resets"] == 1
    buf = io.BytesIO()
    m1.save_to(buf, chunk_bytes=1 << 20)
    tail1 = steps(a1, m1, [2])
    a1.reset_parameters()                              # reset #2: draw 1
    a2, _unused = fresh()
    a2.restore(str(tmp_path / "agent.ck"))
    assert a2.resets == 1
    buf.seek(0)
    m2 = ReplayMemory.load_from(buf, torch.device("cuda:0"), chunk_bytes=1 << 20)
    tail2 = steps(a2, m2, [2])
    a2.reset_parameters()
    assert a1.resets == a2.resets == 2
    assert np.array_equal(tail1, tail2)
    same_agents(a1, a2, "resumed")
    fresh_draw = snapshot(a2)["p"]
    a2.reset_parameters(rng=(0, 0))                    # (draw 0 again: another phi than draw 1 gave)
    assert not np.array_equal(snapshot(a2)["p"][head_mask(a2)], fresh_draw[head_mask(a2)])
    old = {k: v for k, v in ck.items() if k != "resets"}
    a2.restore(old)                                    # a checkpoint from before the counter existed
    assert a2.resets == 0
