"""GPU parity tests of the learn step through the C ABI of librainbow_hip.so against the REAL
reference's golden vectors, and of the drop-in Python classes against the CPU oracle."""
import types

import numpy as np
import pytest
import torch

import scenarios
from helpers import assert_learn_trace_matches, load_golden
from oracle import learner_oracle as O
from oracle.replay_oracle import ReplayOracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("fused_dw", [False, True], ids=["stored-dw", "fused-dw"])
@pytest.mark.parametrize("name", sorted(scenarios.LEARN_CONFIGS))
def test_learn_step_hip_matches_reference_golden(hip, name, fused_dw):
    from cabi_adapter import CAbiLearnAdapter, TorchMem
    from rainbow_amd import _lib as L
    ad = CAbiLearnAdapter(hip, TorchMem(), name)
    ad.learner_flags = (L.LEARNER_FUSE_FC_H_DW | L.LEARNER_WRITE_FUSED_GRADS) if fused_dw else 0
    trace = scenarios.learn_scenario(ad, name, O)
    assert_learn_trace_matches(trace, load_golden("learn_%s.npz" % name), label="hip/" + name)
    ad.close()


def test_intermediates_match_oracle(hip):
    """m (projection), a* (double-Q argmax), pns_a and log p(s,a) against the oracle on the corner-case batch."""
    from cabi_adapter import CAbiLearnAdapter, TorchMem
    name = "canon"
    c = scenarios.LEARN_CONFIGS[name]
    cfg = O.Config(**c)
    ad = CAbiLearnAdapter(hip, TorchMem(), name)
    online, target = O.init_params(cfg, 77), O.init_params(cfg, 78)
    ad.load(online, target)
    rs = np.random.RandomState(5)
    draws = O.noise_draw_count(cfg)
    raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
    ad.reset_noise_online(raw_on)
    batch = scenarios.make_batch(c, 123)
    ad.learn_step(batch, raw_tg)
    want = O.learn(cfg, online, target, O.make_noise(cfg, raw_on), O.make_noise(cfg, raw_tg), batch)
    B, Z = c["batch"], c["atoms"]
    assert np.array_equal(ad.debug(2, (B,), np.int32), want["a_star"].astype(np.int32))
    np.testing.assert_allclose(ad.debug(1, (B, Z), np.float32), want["m"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(ad.debug(1, (B, Z), np.float32).sum(1), 1.0, rtol=1e-5)
    np.testing.assert_allclose(ad.debug(3, (B, Z), np.float32), want["pns_a"], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(ad.debug(0, (B, Z), np.float32), want["log_ps_a"], rtol=1e-5, atol=1e-5)
    ad.close()


def _args(**kw):
    base = dict(device=torch.device("cuda:0"), history_length=4, discount=0.99, multi_step=3, priority_weight=0.4,
                priority_exponent=0.5, atoms=51, V_min=-10.0, V_max=10.0, batch_size=8, norm_clip=10.0, model=None,
                learning_rate=6.25e-5, adam_eps=1.5e-4, architecture="canonical", hidden_size=64, noisy_std=0.1)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("hidden,batch,cap,appends", [(64, 8, 1024, 1500), (512, 32, 4096, 6000)],
                         ids=["small", "baseline-cfg2-h512-b32"])
def test_agent_and_memory_classes_end_to_end_vs_oracle(hip, tmp_path, hidden, batch, cap, appends):
    """The drop-in classes (Agent.learn(mem) on the device-resident fast path: zero-copy frames, noise riding in the
    sampler launch, fused priority write-back, one-pass clip + Adam — exactly what bench.py times) against oracle replay +
    oracle learner for several consecutive steps with injected sampler uniforms and noise; then save/load.  The second
    parametrisation is BASELINE config 2's network and batch (canonical, hidden 512, batch 32, 6 actions)."""
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    args = _args(hidden_size=hidden, batch_size=batch)
    A, B = 6, args.batch_size
    env = types.SimpleNamespace(action_space=lambda: A)
    torch.manual_seed(3)
    agent = Agent(args, env)
    mem = ReplayMemory(args, cap, seed=11)
    ora_mem = ReplayOracle(cap)
    rs = np.random.RandomState(21)
    for _ in range(appends):
        st = rs.randint(0, 256, size=(4, 84, 84)).astype(np.float32) / np.float32(255)
        a, r, term = int(rs.randint(0, A)), float(rs.choice([-1.0, 0.0, 1.0])), bool(rs.random_sample() < 0.02)
        mem.append(torch.from_numpy(st).cuda(), a, r, term)
        ora_mem.append(st, a, r, term)
    cfg = O.Config(batch=B, atoms=51, actions=A, history=4, hidden=hidden, architecture="canonical", multi_step=3)
    online = {k: v.cpu().numpy() for k, v in agent.state_dict().items() if "epsilon" not in k}
    target = {k: v.copy() for k, v in online.items()}
    adam = O.AdamOracle(online, args.learning_rate, args.adam_eps)
    draws = O.noise_draw_count(cfg)
    for step in range(4):
        raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
        uu = rs.random_sample((32, B))
        beta = 0.4 + 0.1 * step
        mem.priority_weight = beta
        ora_mem.priority_weight = beta
        agent.reset_noise(torch.from_numpy(raw_on))
        agent.learn(mem, _target_raw_normals=torch.from_numpy(raw_tg), _unit_uniforms=torch.from_numpy(uu))
        batch = ora_mem.sample_with_uniforms(B, uu)
        want = O.learn(cfg, online, target, O.make_noise(cfg, raw_on), O.make_noise(cfg, raw_tg), batch)
        total, clipped = O.clip_grads(want["grads"], args.norm_clip)
        online = adam.step(clipped)
        ora_mem.update_priorities(batch["tree_idxs"], want["loss"])
        torch.cuda.synchronize()
        assert np.array_equal(mem._out[B]["tree_idxs"].cpu().numpy(), batch["tree_idxs"]), "step %d" % step
        np.testing.assert_allclose(agent._loss.cpu().numpy(), want["loss"], rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(float(agent._norm.item()), total, rtol=2e-5)
        got = {k: v.cpu().numpy() for k, v in agent.state_dict().items() if "epsilon" not in k}
        for k in online:
            np.testing.assert_allclose(got[k], online[k], rtol=0, atol=3e-7, err_msg="step %d %s" % (step, k))
        if step == 1:
            agent.update_target_net()
            target = {k: v.copy() for k, v in online.items()}
    # tree after 4 priority updates matches the oracle's to ~1 ulp (loss^0.5 is a float32 pow)
    np.testing.assert_allclose(mem._dump()["tree"], ora_mem.transitions.tree, rtol=2e-5)
    # act / evaluate_q, train vs eval mode
    st = rs.randint(0, 256, size=(4, 84, 84)).astype(np.float32) / np.float32(255)
    noise_on = O.make_noise(cfg, raw_on)
    a_want, q_want = O.act(cfg, online, noise_on, st)
    assert agent.act(torch.from_numpy(st).cuda()) == a_want
    np.testing.assert_allclose(agent.evaluate_q(torch.from_numpy(st).cuda()), q_want, rtol=2e-5, atol=1e-6)
    agent.eval()
    a_want, q_want = O.act(cfg, online, None, st)
    assert agent.act(torch.from_numpy(st).cuda()) == a_want
    # (q is an expectation over a [-10, 10] support that nearly cancels at initialisation: absolute floor 1e-6)
    np.testing.assert_allclose(agent.evaluate_q(torch.from_numpy(st).cuda()), q_want, rtol=2e-5, atol=1e-6)
    agent.train()
    # vectorised actors: act_batch(states)[i] == act(states[i]) (batched forward through the training kernels)
    sts = torch.from_numpy(rs.randint(0, 256, size=(5, 4, 84, 84)).astype(np.float32) / np.float32(255)).cuda()
    assert list(agent.act_batch(sts)) == [agent.act(s) for s in sts]
    many = sts.repeat(4, 1, 1, 1)[:19]                       # more than 2 * batch_size states: processed in chunks
    assert list(agent.act_batch(many)) == [agent.act(s) for s in many]
    # checkpoint interchange: reference key names, round trip (agent.py:26-36,106-107)
    agent.save(str(tmp_path), "model.pth")
    sd = torch.load(str(tmp_path / "model.pth"), map_location="cpu")
    assert list(sd.keys())[:12] == ["convs.0.weight", "convs.0.bias", "convs.2.weight", "convs.2.bias", "convs.4.weight",
                                    "convs.4.bias", "fc_h_v.weight_mu", "fc_h_v.weight_sigma", "fc_h_v.bias_mu",
                                    "fc_h_v.bias_sigma", "fc_h_v.weight_epsilon", "fc_h_v.bias_epsilon"]
    assert tuple(sd["fc_h_v.weight_epsilon"].shape) == (hidden, 3136) and tuple(sd["fc_z_a.bias_epsilon"].shape) == (A * 51,)
    args2 = _args(model=str(tmp_path / "model.pth"), hidden_size=hidden, batch_size=B)
    agent2 = Agent(args2, env)
    for k, v in agent2.state_dict().items():
        if "epsilon" not in k:
            assert torch.equal(v.cpu(), sd[k]), k


AGENT_SHAPES = {
    # name: (architecture, hidden, batch, actions, multi_step, replay capacity, appends, data seed)
    "baseline-cfg2-h512-b32-a6": ("canonical", 512, 32, 6, 3, 4096, 6000, 31),
    "baseline-cfg3-h512-b256-a4": ("canonical", 512, 256, 4, 3, 8192, 12000, 31),
    "baseline-cfg4-dataeff-h256-n20": ("data-efficient", 256, 32, 6, 20, 16384, 20000, 31),
    # above batch 256: the 1024-thread sampler variant (k_sample<1024, ...> drawing 320 samples), the pending optimiser pass as a launch
    # of its own in front of it (optimizer_host.h attach_pending_pass: batch > 256 is not hosted) and the priority write-back
    # outside the hidden layer's launch (learner_plan.h plan_fc_bwd: up_enabled needs B <= 256)
    "dataeff-h256-b320-a6": ("data-efficient", 256, 320, 6, 3, 8192, 12000, 31),
}
AGENT_STEPS = 6
RELU_MARGIN = 3e-8      # ~10x the f32 rounding noise of a hidden pre-activation (oracle.learner_oracle.learn: hidden_relu_margin)


def agent_shape_inputs(shape):
    """The seeded inputs of the class-level test below: transitions for the replay and, per step, the injected randomness."""
    arch, hidden, B, A, n, cap, appends, seed = AGENT_SHAPES[shape]
    rs = np.random.RandomState(seed)
    pool = rs.randint(0, 256, size=(64, 84, 84)).astype(np.uint8)
    term = rs.random_sample(appends) < 0.01
    acts = rs.randint(0, A, appends)
    rews = rs.choice([-1.0, 0.0, 1.0], size=appends).astype(np.float32)
    fidx = rs.randint(0, 64, appends)
    cfg = O.Config(batch=B, atoms=51, actions=A, history=4, hidden=hidden, architecture=arch, multi_step=n)
    draws = O.noise_draw_count(cfg)
    steps = [dict(raw_on=rs.randn(draws).astype(np.float32), raw_tg=rs.randn(draws).astype(np.float32),
                  uu=rs.random_sample((64, B)), beta=0.4 + 0.05 * k) for k in range(AGENT_STEPS)]
    return dict(cfg=cfg, pool=pool, term=term, acts=acts, rews=rews, fidx=fidx, steps=steps)


def agent_shape_oracle(shape, online, args, inp=None):
    """The oracle's side of that test (CPU only: oracle replay + oracle learner + torch Adam): per step the batch, loss,
    norm and post-Adam parameters; the final tree.  `online` = the agent's initial parameters."""
    arch, hidden, B, A, n, cap, appends, _seed = AGENT_SHAPES[shape]
    inp = inp or agent_shape_inputs(shape)
    cfg = inp["cfg"]
    ora_mem = ReplayOracle(cap, multi_step=n)
    for i in range(appends):
        ora_mem.append_frame(inp["pool"][inp["fidx"][i]], int(inp["acts"][i]), float(inp["rews"][i]), bool(inp["term"][i]))
    target = {k: v.copy() for k, v in online.items()}
    adam = O.AdamOracle(online, args.learning_rate, args.adam_eps)
    out = []
    for k, st in enumerate(inp["steps"]):
        ora_mem.priority_weight = st["beta"]
        batch = ora_mem.sample_with_uniforms(B, st["uu"])
        want = O.learn(cfg, online, target, O.make_noise(cfg, st["raw_on"]), O.make_noise(cfg, st["raw_tg"]), batch)
        total, clipped = O.clip_grads(want["grads"], args.norm_clip)
        online = adam.step(clipped)
        ora_mem.update_priorities(batch["tree_idxs"], want["loss"])
        out.append(dict(tree_idxs=batch["tree_idxs"], loss=want["loss"], norm=total, margin=want["hidden_relu_margin"],
                        params={k2: v.copy() for k2, v in online.items()}))
        if k == 2:
            target = {k2: v.copy() for k2, v in online.items()}
    return out, ora_mem.transitions.tree


P_ATOL_B256 = 1.5e-6    # batch 256, six steps, ReLU decisions equal: plain absolute tolerance on EVERY post-Adam parameter element
                        # (seen: 1.03e-6 on one conv weight at step 4; round 5 allowed 0.5 % of a tensor up to 6e-6 on top of this bulk bound)


class _MaskedOracle:
    """agent_shape_oracle one step at a time, the hidden layer's ReLU decisions of the differentiated forward taken from the
    device (oracle learn(hidden_mask=...)): per step the batch, loss, norm, post-Adam parameters, and how many decisions differed
    from the oracle's own and on how small a pre-activation."""

    def __init__(self, shape, online, args, inp):
        arch, hidden, B, A, n, cap, appends, _seed = AGENT_SHAPES[shape]
        self.B, self.args, self.inp, self.cfg = B, args, inp, inp["cfg"]
        self.mem = ReplayOracle(cap, multi_step=n)
        for i in range(appends):
            self.mem.append_frame(inp["pool"][inp["fidx"][i]], int(inp["acts"][i]), float(inp["rews"][i]), bool(inp["term"][i]))
        self.online = online
        self.target = {k: v.copy() for k, v in online.items()}
        self.adam = O.AdamOracle(online, args.learning_rate, args.adam_eps)

    def step(self, k, device_mask):
        st = self.inp["steps"][k]
        self.mem.priority_weight = st["beta"]
        batch = self.mem.sample_with_uniforms(self.B, st["uu"])
        want = O.learn(self.cfg, self.online, self.target, O.make_noise(self.cfg, st["raw_on"]), O.make_noise(self.cfg, st["raw_tg"]),
                       batch, hidden_mask=device_mask)
        total, clipped = O.clip_grads(want["grads"], self.args.norm_clip)
        self.online = self.adam.step(clipped)
        self.mem.update_priorities(batch["tree_idxs"], want["loss"])
        if k == 2:
            self.target = {k2: v.copy() for k2, v in self.online.items()}
        return dict(tree_idxs=batch["tree_idxs"], loss=want["loss"], norm=total, margin=want["hidden_relu_margin"],
                    flips=want["hidden_mask_flips"], flip_abs=want["hidden_mask_flip_abs"],
                    params={k2: v.copy() for k2, v in self.online.items()})

    def tree(self):
        return self.mem.transitions.tree


def _assert_params_track(got, want, atol, flip_atol, flip_frac, msg):
    """Post-Adam parameters: every element within `atol`, except that a fraction `flip_frac` of a tensor's elements may deviate up
    to `flip_atol` (batch 256 only, see the test's docstring; flip_frac = 0 is a plain absolute tolerance)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    bad = d > atol
    assert float(d.max()) <= flip_atol and int(bad.sum()) <= int(flip_frac * d.size), \
        "%s: %d / %d elements beyond %.1e (allowed %d), largest %.3e (allowed %.1e)" % (
            msg, int(bad.sum()), d.size, atol, int(flip_frac * d.size), float(d.max()), flip_atol)


@pytest.mark.parametrize("shape", sorted(AGENT_SHAPES))
def test_agent_default_flag_set_with_hosted_optimiser_pass_vs_oracle(hip, shape):
    """The EXACT configuration bench.py times at BASELINE configs 2, 3 and 4 — and one shape above batch 256, where the pending
    pass is NOT hosted: the sampler launch takes no tenants beyond 256 samples, so call k + 1 runs call k's pass as a launch of its
    own in front of its sampler, and the priority write-back is a launch of its own as well; everything below about reading the
    parameters raw after call k + 1 holds there unchanged — against the oracle (agent.py:61-100,
    memory.py:124-159): `Agent` with its defaults — RB_LEARNER_DEFER_UPDATE (+ RB_LEARNER_IMPLICIT_SIGMA where the hidden
    layer is large enough) — so that the clip + Adam pass of learn call k runs as tenant workgroups of call k + 1's SAMPLER
    launch (k_sample<1024, 4> hosting the paired (mu, sigma) optimiser body; 256 samples at config 3, where the backward is
    k_fc_gemm_bwd with the implicit sigma gradient; 24-slot windows at config 4, the hosting limit), zero-copy frames, fused
    priority write-back.  Sampler uniforms and both nets' noise are injected (the injected target draw overwrites the
    device-RNG draw the hosting launch carries).  Six consecutive learn() calls with one update_target_net():
    per-sample loss and tree indices at every step; the parameters and the norm of step k are read RAW (no flush) after
    call k + 1 has hosted that step's pass — reading them through the public names would run the pass as a launch of its
    own and the hosted path would never be exercised; the tree at the end.
    Parameter tolerance: 3e-7 absolute at batch 32 (as the two-step tests).
    Batch 256 (no blanket widening): the hidden layer there is a split-K GEMM whose pre-activations carry
    ~5e-8 of summation-order noise, and the smallest |pre-activation| among a step's 262 144 is ~3e-8 on any seed, so every few
    steps one (sample, unit) ReLU decision differs from the oracle's — relu' is a step, the reference itself is only defined up
    to its GEMM's summation order there — and that one decision moves that sample's contribution to EVERY upstream gradient
    (seen in round 5: 1 of 512 elements of fc_h_a.bias_mu off by 2.1e-6, 33 of 32 768 of a conv weight by 5.9e-7).  The test
    now PROVES that this is all there is: after every learn() it reads the device's hidden activations (rb_learner_debug_read 5,
    no flush), hands the oracle the device's ReLU decisions (oracle learn(hidden_mask=...)), and requires (a) every decision
    that differs from the oracle's own to sit on a pre-activation inside the noise (|pre| < 2e-7 at the first step, where the
    parameters are identical; < 1e-5 later, where they agree within the tolerance below; at most 32 of 262 144 per step),
    and (b) with the decisions equal, EVERY parameter element within the plain absolute tolerance — no fraction of outliers.
    A missing or doubled pass moves every element by ~lr = 6.25e-5."""
    from rainbow_amd import _lib as L
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    arch, hidden, B, A, n, cap, appends, _seed = AGENT_SHAPES[shape]
    big = B > 32
    p_atol, flip_atol, flip_frac = (3e-7, 3e-7, 0.0) if not big else (P_ATOL_B256, P_ATOL_B256, 0.0)
    n_rtol = 5e-5            # (helpers.assert_learn_trace_matches: the reference's own f32 norm is 2e-5 from exact)
    args = _args(architecture=arch, hidden_size=hidden, batch_size=B, multi_step=n)
    env = types.SimpleNamespace(action_space=lambda: A)
    torch.manual_seed(5)
    agent = Agent(args, env)
    assert agent._defer_update and agent._step_dev is not None
    mem = ReplayMemory(args, cap, seed=13)
    inp = agent_shape_inputs(shape)
    for lo in range(0, appends, 2000):
        hi = min(appends, lo + 2000)
        mem.append_batch(torch.from_numpy(inp["pool"][inp["fidx"][lo:hi]]).cuda(), inp["acts"][lo:hi], inp["rews"][lo:hi],
                         inp["term"][lo:hi])
    online0 = {k: v.cpu().numpy() for k, v in agent.state_dict().items() if "epsilon" not in k}
    if big:      # the oracle runs step by step BEHIND the device, with the device's hidden-layer ReLU decisions (docstring)
        want, stepper = [], _MaskedOracle(shape, online0, args, inp)
    else:
        want, want_tree = agent_shape_oracle(shape, online0, args, inp)
        assert min(w["margin"] for w in want) > RELU_MARGIN, \
            "ill-conditioned seed: a hidden pre-activation within rounding noise of 0 (tools/precheck_agent_shapes.py)"
    h_buf = torch.empty(B, 2 * hidden, dtype=torch.float32, device="cuda")

    def raw_params():      # the borrowed flat buffer as it is NOW (a pending pass is NOT run)
        torch.cuda.synchronize()
        return {name: agent._view(agent._params, name).cpu().numpy() for name, _o, _s in agent._layout}

    hosted = 0
    for step, st in enumerate(inp["steps"]):
        mem.priority_weight = st["beta"]
        agent.reset_noise(torch.from_numpy(st["raw_on"]))
        was_pending = agent._update_pending
        agent.learn(mem, _target_raw_normals=torch.from_numpy(st["raw_tg"]), _unit_uniforms=torch.from_numpy(st["uu"]))
        if big:
            L.check(agent._lib, agent._lib.rb_learner_debug_read(agent._h, 5, h_buf.data_ptr(), agent._stream()))   # (no flush: see the header)
            torch.cuda.synchronize()
            want.append(stepper.step(step, h_buf.cpu().numpy() > 0))
            # step 0: identical parameters, so only the summation order differs (~5e-8 on a pre-activation); later steps: the
            # parameters agree within P_ATOL_B256, a 3136-term dot product of them within ~1e-6 typically
            assert want[-1]["flips"] <= 32 and want[-1]["flip_abs"] < (2e-7 if step == 0 else 1e-5), \
                "step %d: %d ReLU decisions differ from the oracle's own, the largest on |pre| = %.3e" % (step, want[-1]["flips"], want[-1]["flip_abs"])
        if was_pending:
            assert agent._update_pending, "step %d" % step
            hosted += 1
            got = raw_params()      # = the parameters after step - 1's update, which this call's sampler launch hosted (above batch 256: which this call ran in front of its sampler)
            prev = want[step - 1]
            for k in prev["params"]:
                _assert_params_track(got[k], prev["params"][k], p_atol, flip_atol, flip_frac, "hosted pass of step %d: %s" % (step - 1, k))
            np.testing.assert_allclose(float(agent._norm_buf.item()), prev["norm"], rtol=n_rtol)
        torch.cuda.synchronize()
        assert np.array_equal(mem._out[B]["tree_idxs"].cpu().numpy(), want[step]["tree_idxs"]), "step %d" % step
        np.testing.assert_allclose(agent._loss.cpu().numpy(), want[step]["loss"], rtol=2e-5, atol=1e-6, err_msg="step %d" % step)
        if step == 2:      # update_target_net runs the pending pass as a launch of its own (every entry point does)
            agent.update_target_net()
            agent._update_pending = False
    assert hosted >= 4, hosted
    if big:
        want_tree = stepper.tree()
        print(shape, "ReLU decisions that differed from the oracle's own, per step:", [(w["flips"], "%.1e" % w["flip_abs"]) for w in want])
    got = {k: v.cpu().numpy() for k, v in agent.state_dict().items() if "epsilon" not in k}      # (flushes the last pass)
    for k in got:
        _assert_params_track(got[k], want[-1]["params"][k], p_atol, flip_atol, flip_frac, "final %s" % k)
    np.testing.assert_allclose(float(agent._norm.item()), want[-1]["norm"], rtol=n_rtol)
    np.testing.assert_allclose(mem._dump()["tree"], want_tree, rtol=2e-5)
    assert int(agent.optimiser.state_dict()["state"][0]["step"]) == AGENT_STEPS


def test_compat_path_with_foreign_replay(hip):
    """Agent.learn(mem) with a replay object that only offers the reference's sample()/update_priorities()."""
    from rainbow_amd.agent import Agent
    args = _args(architecture="data-efficient", hidden_size=32, batch_size=6)
    env = types.SimpleNamespace(action_space=lambda: 4)
    agent = Agent(args, env)
    c = dict(scenarios.LEARN_CONFIGS["dataeff"])
    batch = scenarios.make_batch(c, 5)

    class Foreign:
        def sample(self, B):
            f = lambda a: torch.from_numpy(a).to(torch.float32).div_(255).cuda()
            return (np.arange(B), f(batch["states"]), torch.from_numpy(batch["actions"]).cuda(),
                    torch.from_numpy(batch["returns"]).cuda(), f(batch["next_states"]),
                    torch.from_numpy(batch["nonterminals"]).reshape(-1, 1).cuda(), torch.from_numpy(batch["weights"]).cuda())

        def update_priorities(self, idxs, prios):
            self.got = (idxs, prios)

    fm = Foreign()
    agent.learn(fm)
    assert isinstance(fm.got[1], np.ndarray) and fm.got[1].shape == (6,) and np.all(np.isfinite(fm.got[1]))
    assert np.all(fm.got[1] > 0)


@pytest.mark.parametrize("base", ["dataeff", "canon"])
def test_wide_batch_matches_oracle(hip, monkeypatch, base):
    """Batch 64 (128 online rows): the noisy-linear forward switches to 64-row m-chunks (k_nl_fwd3<4>) and the conv
    weight-gradient workgroups sum two images each; loss and every gradient against the oracle on the same inputs."""
    from cabi_adapter import CAbiLearnAdapter, TorchMem
    cfgd = dict(scenarios.LEARN_CONFIGS[base], batch=64, multi_step=3)
    monkeypatch.setitem(scenarios.LEARN_CONFIGS, "wide", cfgd)
    cfg = O.Config(**cfgd)
    ad = CAbiLearnAdapter(hip, TorchMem(), "wide")
    online, target = O.init_params(cfg, 177), O.init_params(cfg, 178)
    ad.load(online, target)
    rs = np.random.RandomState(15)
    draws = O.noise_draw_count(cfg)
    raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
    ad.reset_noise_online(raw_on)
    batch = scenarios.make_batch(cfgd, 321)
    got = ad.learn_step(batch, raw_tg)
    want = O.learn(cfg, online, target, O.make_noise(cfg, raw_on), O.make_noise(cfg, raw_tg), batch)
    np.testing.assert_allclose(got["loss"], want["loss"], rtol=2e-5, atol=1e-6)
    for k, g in want["grads"].items():
        scale = float(np.max(np.abs(g))) if g.size else 0.0
        np.testing.assert_allclose(got["grads"][k], g, rtol=2e-4, atol=5e-6 * scale + 1e-9, err_msg=k)
    ad.close()


# BASELINE.json configs 2, 3, 4 — the shapes bench.py times.  At these shapes the step runs code no
# small fixture reaches: the 4-way row split of the hidden layer's input gradient + k_dfeat_finish(splits=4) (H = 512),
# 64-row m-chunks and image-group sums (B = 256), the n = 20 data-efficient network at hidden 256.
BASELINE_SHAPES = {
    "cfg2-canonical-h512-b32-a6": dict(architecture="canonical", hidden=512, actions=6, atoms=51, batch=32, multi_step=3,
                                       discount=0.99, history=4, v_min=-10.0, v_max=10.0),
    "cfg3-canonical-h512-b256-a4": dict(architecture="canonical", hidden=512, actions=4, atoms=51, batch=256, multi_step=3,
                                        discount=0.99, history=4, v_min=-10.0, v_max=10.0),
    "cfg4-dataeff-h256-n20-b32-a6": dict(architecture="data-efficient", hidden=256, actions=6, atoms=51, batch=32,
                                         multi_step=20, discount=0.99, history=4, v_min=-10.0, v_max=10.0),
}


@pytest.mark.parametrize("shape", ["cfg2-canonical-h512-b32-a6", "cfg3-canonical-h512-b256-a4"])
def test_conv_block_orders_match_oracle(hip, monkeypatch, shape):
    """The conv launches' block order is a placement decision (which XCD's L2 holds a layer's input), never a numerical one:
    the (chunk, tile, image) order that remains the fallback when the image count is not a multiple of 8 (RB_OPTS=img_fast=0)
    against the oracle at the shapes the bench times; the default image-fastest order is what every other test of this file
    runs."""
    monkeypatch.setenv("RB_OPTS", "img_fast=0")
    test_learn_step_at_baseline_shapes_matches_oracle(hip, monkeypatch, shape, False)


@pytest.mark.parametrize("fused_dw", [False, True], ids=["stored-dw", "fused-dw"])
@pytest.mark.parametrize("shape", sorted(BASELINE_SHAPES))
def test_learn_step_at_baseline_shapes_matches_oracle(hip, monkeypatch, shape, fused_dw):
    """TWO consecutive learn steps through the C ABI at the exact network / batch of each BASELINE config against the CPU
    oracle on the same inputs: per-sample loss, global gradient norm, all 22 (clipped) gradients and the post-Adam
    parameters, with the tolerances of helpers.assert_learn_trace_matches (agent.py:61-100)."""
    from cabi_adapter import CAbiLearnAdapter, TorchMem
    cfgd = BASELINE_SHAPES[shape]
    monkeypatch.setitem(scenarios.LEARN_CONFIGS, shape, cfgd)
    cfg = O.Config(**cfgd)
    hy = scenarios.LEARN_HYPER
    ad = CAbiLearnAdapter(hip, TorchMem(), shape)
    if fused_dw:   # the Agent's configuration: fc_h weight gradient recomputed inside the clip + Adam pass (batch <= 32);
        from rainbow_amd import _lib as L      # WRITE_FUSED_GRADS makes that pass store what it computed, for this comparison
        ad.learner_flags = L.LEARNER_FUSE_FC_H_DW | L.LEARNER_WRITE_FUSED_GRADS
    online, target = O.init_params(cfg, 901), O.init_params(cfg, 902)
    ad.load(online, target)
    adam = O.AdamOracle(online, hy["lr"], hy["adam_eps"])
    draws = O.noise_draw_count(cfg)
    rs = np.random.RandomState(55)
    got_t, want_t = {}, {}
    for k in range(2):
        raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
        ad.reset_noise_online(raw_on)
        batch = scenarios.make_batch(cfgd, 700 + k)
        got = ad.learn_step(batch, raw_tg)
        want = O.learn(cfg, online, target, O.make_noise(cfg, raw_on), O.make_noise(cfg, raw_tg), batch)
        total, clipped = O.clip_grads(want["grads"], hy["norm_clip"])
        online = adam.step(clipped)
        got_t["s%d_loss" % k], want_t["s%d_loss" % k] = got["loss"], want["loss"]
        got_t["s%d_grad_norm" % k], want_t["s%d_grad_norm" % k] = np.float32(got["grad_norm"]), np.float32(total)
        exact = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in want["grads"].values()))
        if exact <= hy["norm_clip"]:   # device norm against the EXACT norm of the oracle's gradients (f64), tightly
            np.testing.assert_allclose(got["grad_norm"], exact, rtol=2e-6)
        for name in clipped:
            got_t["s%d_grad/%s" % (k, name)], want_t["s%d_grad/%s" % (k, name)] = got["grads"][name], clipped[name]
        for name, p in ad.params().items():
            got_t["s%d_param/%s" % (k, name)], want_t["s%d_param/%s" % (k, name)] = p, online[name]
        if k == 0:
            B, Z = cfgd["batch"], cfgd["atoms"]
            assert np.array_equal(ad.debug(2, (B,), np.int32), want["a_star"].astype(np.int32))
            np.testing.assert_allclose(ad.debug(1, (B, Z), np.float32), want["m"], rtol=1e-4, atol=1e-6)
    assert_learn_trace_matches(got_t, want_t, label="hip/" + shape)
    ad.close()


def test_tiled_gemm_hidden_layer_tracks_the_streamed_kernels_over_many_steps(hip, monkeypatch):
    """BASELINE config 3's shape (canonical net, batch 256): 40 consecutive learn steps with the hidden layer on the tiled GEMMs
    of fc_gemm.h (split-K partial tiles, the self-resetting arrival counters of 48 output tiles, two workgroups per CU in the
    backward) against a twin on the streamed noisy-linear kernels (RB_OPTS fc_gemm=0) fed the same batches and noise: the two
    differ only in the order of their f32 sums, so every per-sample loss, the norm and the parameters stay close all the way
    (1e-3 / 2e-3 relative, 5e-5 absolute on the parameters) — a lost or doubly counted partial tile would show at once, and the
    counters must come back to zero after every launch for the next one to work."""
    from cabi_adapter import CAbiLearnAdapter, TorchMem
    shape = "cfg3-canonical-h512-b256-a4"
    cfgd = BASELINE_SHAPES[shape]
    monkeypatch.setitem(scenarios.LEARN_CONFIGS, shape, cfgd)
    cfg = O.Config(**cfgd)
    online, target = O.init_params(cfg, 911), O.init_params(cfg, 912)
    ads = []
    for opts in ("fc_gemm=-1", "fc_gemm=0"):
        monkeypatch.setenv("RB_OPTS", opts)
        ad = CAbiLearnAdapter(hip, TorchMem(), shape)
        ad.load(online, target)
        ads.append(ad)
    draws = O.noise_draw_count(cfg)
    rs = np.random.RandomState(56)
    for k in range(40):
        raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
        batch = scenarios.make_batch(cfgd, 800 + k)
        outs = []
        for ad in ads:
            ad.reset_noise_online(raw_on)
            outs.append(ad.learn_step(batch, raw_tg))
        a, b = outs
        # (two f32 summation orders drift apart as the steps feed on each other: 8.5e-5 on the norm after ten steps; a lost tile
        # is an O(1) error in the same quantities)
        np.testing.assert_allclose(a["loss"], b["loss"], rtol=1e-3, atol=1e-4, err_msg="step %d" % k)
        np.testing.assert_allclose(a["grad_norm"], b["grad_norm"], rtol=2e-3, err_msg="step %d" % k)
    pa, pb = ads[0].params(), ads[1].params()
    for name in pa:
        np.testing.assert_allclose(pa[name], pb[name], rtol=0, atol=5e-5, err_msg=name)   # (Adam turns a near-zero gradient of either sign into +-lr: 9e-6 seen)
    for ad in ads:
        ad.close()


def test_device_rng_noise_statistics(hip):
    """The PRODUCTION noise path (rb_learner_reset_noise with raw = NULL: device Philox + Box-Muller, then
    f(x) = sign(x) sqrt|x|, model.py:32-40): >= 10^6 values, moments and a Kolmogorov-Smirnov distance against the exact
    law of f(N(0,1)); the three `which` modes consume distinct Philox epochs (no two resamples ever repeat)."""
    import math
    from cabi_adapter import CAbiLearnAdapter, TorchMem
    from scipy import stats
    name = "cfg2-canonical-h512-b32-a6"
    scenarios.LEARN_CONFIGS[name] = BASELINE_SHAPES[name]
    try:
        ad = CAbiLearnAdapter(hip, TorchMem(), name)
    finally:
        del scenarios.LEARN_CONFIGS[name]
    from rainbow_amd import _lib as L
    m = ad.mem
    n_noise = ad.n_noise
    layout = cabi_noise_layout(hip, ad.cfg)
    live = np.zeros(n_noise, dtype=bool)
    for _name, (off, shape) in layout.items():
        live[off:off + shape[0]] = True
    draws, seen = [], []
    for rep in range(130):                            # 130 x 8.7k values > 10^6
        which = rep % 3
        L.check(hip, hip.rb_learner_reset_noise(ad.h, which, None, m.stream))
        m.sync()
        z_on, z_tg = m.download(ad.z_on)[live], m.download(ad.z_tg)[live]
        fresh = {0: [z_on], 1: [z_tg], 2: [z_on, z_tg]}[which]
        for v in fresh:
            draws.append(v.copy())
            key = v[:64].tobytes()
            assert key not in seen, "a noise resample repeated an earlier epoch's values (rep %d, which %d)" % (rep, which)
            seen.append(key)
        if which == 2:
            assert not np.array_equal(z_on, z_tg)
    x = np.concatenate(draws).astype(np.float64)
    assert x.size >= 1_000_000
    g = np.sign(x) * x * x                            # invert f: g ~ N(0,1) if and only if x ~ f(N(0,1))
    n = g.size
    assert abs(g.mean()) < 5.0 / math.sqrt(n)
    assert abs(g.var() - 1.0) < 5.0 * math.sqrt(2.0 / n)
    assert abs((g ** 4).mean() - 3.0) < 5.0 * math.sqrt(96.0 / n)
    assert abs((g ** 3).mean()) < 5.0 * math.sqrt(15.0 / n)
    d, _p = stats.kstest(g, "norm")
    assert d < 1.95 / math.sqrt(n), d                 # KS critical value at alpha ~ 1e-3
    # E|f(x)| = E sqrt|N| = 2^(1/4) Gamma(3/4) / sqrt(pi)
    want = 2 ** 0.25 * math.gamma(0.75) / math.sqrt(math.pi)
    assert abs(np.abs(x).mean() - want) < 5.0 * math.sqrt((math.sqrt(2 / math.pi) - want ** 2) / n)
    # independence across positions and epochs: lag-1 autocorrelation and epoch-to-epoch correlation ~ 0
    assert abs(np.corrcoef(g[:-1], g[1:])[0, 1]) < 5.0 / math.sqrt(n)
    a, b = draws[0].astype(np.float64), draws[3].astype(np.float64)
    assert abs(np.corrcoef(a, b)[0, 1]) < 5.0 / math.sqrt(a.size)
    ad.close()


def cabi_noise_layout(lib, cfg):
    from cabi_adapter import query_layout
    return query_layout(lib, cfg, lib.rb_learner_noise_layout)


def test_reference_written_checkpoint_interchange(hip, tmp_path):
    """tests/golden/ref_model_dataeff.pth was written by the REFERENCE's Agent.save (tests/golden/make_golden_model.py).
    Loading it through args.model (agent.py:26-36) must reproduce the reference's own act / evaluate_q on the same
    states in train mode (i.e. with the checkpoint's epsilon buffers: no resample after load) and eval mode; saving it
    back must give a file the reference layout-checks as identical: same keys, same order, bit-identical tensors."""
    import os
    from helpers import GOLDEN_DIR
    from rainbow_amd.agent import Agent
    path = os.path.join(GOLDEN_DIR, "ref_model_dataeff.pth")
    want = load_golden("ref_model_dataeff.npz")
    args = _args(architecture="data-efficient", hidden_size=32, batch_size=4, model=path)
    env = types.SimpleNamespace(action_space=lambda: 4)
    agent = Agent(args, env)
    states = torch.from_numpy(want["states_u8"].astype(np.float32) / np.float32(255)).cuda()
    agent.train()
    assert [agent.act(s) for s in states] == list(want["act_train"])
    np.testing.assert_allclose([agent.evaluate_q(s) for s in states], want["q_train"], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(agent.evaluate_q_batch(states), want["q_train"], rtol=2e-5, atol=1e-6)
    assert list(agent.act_batch(states)) == list(want["act_train"])
    agent.eval()
    assert [agent.act(s) for s in states] == list(want["act_eval"])
    np.testing.assert_allclose(agent.evaluate_q_batch(states), want["q_eval"], rtol=2e-5, atol=1e-6)
    agent.train()
    ref_sd = torch.load(path, map_location="cpu")
    agent.save(str(tmp_path), "back.pth")
    back = torch.load(str(tmp_path / "back.pth"), map_location="cpu")
    assert list(back.keys()) == list(ref_sd.keys())
    for k in ref_sd:
        assert back[k].dtype == ref_sd[k].dtype and torch.equal(back[k], ref_sd[k]), k
    # strictness of the reference's load_state_dict (agent.py:33)
    broken = dict(ref_sd)
    broken.pop("fc_z_a.bias_epsilon")
    with pytest.raises(RuntimeError):
        agent.load_state_dict(broken)
    broken = dict(ref_sd, extra_key=torch.zeros(1))
    with pytest.raises(RuntimeError):
        agent.load_state_dict(broken)


def test_batched_evaluation_of_validation_memory(hip):
    """SURVEY 8f row 4 (test.py:38-39): Q over a 500-state validation memory as a handful of launches.  states_at(indices)
    must equal the per-index iterator (memory.py:162-178) and evaluate_q_memory must equal 500 single evaluate_q calls and
    the oracle's act on a sample of the states."""
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    args = _args(hidden_size=64, batch_size=8)
    A, cap = 6, 500
    env = types.SimpleNamespace(action_space=lambda: A)
    torch.manual_seed(9)
    agent = Agent(args, env)
    val = ReplayMemory(args, cap, seed=1)
    rs = np.random.RandomState(2)
    g = torch.Generator(device="cuda").manual_seed(2)
    frames = torch.randint(0, 256, (cap, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
    val.append_batch(frames, np.full(cap, -1), np.zeros(cap), rs.random_sample(cap) < 0.05)     # main.py:134: action -1
    assert val.transitions.full and val.transitions.index == 0
    per_index = torch.stack([s for s in val])                       # the reference's iterator protocol, 500 launches
    batched = val.states_at(torch.arange(cap))
    assert torch.equal(per_index, batched)
    agent.eval()                                                    # test.py evaluates with online_net.eval()
    qs = agent.evaluate_q_memory(val)
    single = np.array([agent.evaluate_q(s) for s in per_index[:40]], dtype=np.float32)
    np.testing.assert_allclose(qs[:40], single, rtol=2e-5, atol=1e-6)
    cfg = O.Config(batch=8, atoms=51, actions=A, history=4, hidden=64, architecture="canonical", multi_step=3)
    online = {k: v.cpu().numpy() for k, v in agent.state_dict().items() if "epsilon" not in k}
    acts = agent.act_batch(batched[:32])
    for i in (0, 1, 17, 31, 499):
        a_want, q_want = O.act(cfg, online, None, per_index[i].cpu().numpy())
        np.testing.assert_allclose(qs[i], q_want, rtol=2e-5, atol=1e-6)
        if i < 32:
            assert acts[i] == a_want
    assert qs.shape == (cap,) and np.all(np.isfinite(qs))


@pytest.mark.parametrize("one_call,spec", [("1", False), ("0", False), ("1", True)],
                         ids=["train_step", "three-calls", "train_step-early-draw"])
def test_deferred_update_agent_is_bit_identical_to_the_undeferred_one(hip, monkeypatch, one_call, spec):
    """Third case, RB_OPTS spec_draw=1: from the third back-to-back learn() on, the priority write-back and the NEXT call's draw run
    on the replay's own stream behind the head kernel, and the next sampler launch accepts the draw (act / target-sync / state_dict
    in between do not touch the replay: the streak goes on) — two streams, in-kernel flags, the same bits.
    RAINBOW_AMD_DEFER_UPDATE (default on): Agent.learn leaves clip + Adam pending and the next learn's sampler launch
    hosts it (include/rainbow_hip.h RB_LEARNER_DEFER_UPDATE).  Against an agent with the switch off (same device-resident
    step number): 8 steps with acting, a target sync and a state_dict() in between — per-step losses, actions, parameters,
    target parameters, Adam moments, the norm and the sum-tree bit-identical; the deferred agent really deferred."""
    import ctypes as C
    from rainbow_amd import _lib as L
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    args = _args(architecture="data-efficient", hidden_size=64, batch_size=16)
    env = types.SimpleNamespace(action_space=lambda: 4)

    def fresh(defer):
        monkeypatch.setenv("RAINBOW_AMD_DEFER_UPDATE", defer)
        # RB_LEARNER_IMPLICIT_SIGMA rides on the deferral (the hosted pass forms the hidden layer's sigma gradient itself and
        # updates (mu, sigma) pairs together); the library switches it on from 1 M-element layers: force it on this small net
        monkeypatch.setenv("RB_OPTS", "implicit_small=1,spec_draw=%d" % (1 if spec and defer == "1" else 0))
        # the deferring agent through rb_learner_train_step or through the step's entry points one by one
        # (rb_learner_attach_pending / rb_learner_clip_adam_deferred: the path the replica exchange uses as well)
        monkeypatch.setenv("RAINBOW_AMD_ONE_CALL", one_call if defer == "1" else "1")
        torch.manual_seed(77)
        np.random.seed(77)
        agent = Agent(args, env)
        if agent._step_dev is None:      # the twin forms its bias corrections on the device as well
            agent._step_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
            L.check(agent._lib, agent._lib.rb_learner_set_step_counter(agent._h, agent._step_dev.data_ptr()))
        mem = ReplayMemory(args, 2048, seed=5)
        g = torch.Generator(device="cuda").manual_seed(3)
        rs = np.random.RandomState(3)
        for _ in range(2):
            mem.append_batch(torch.randint(0, 256, (1500, 84, 84), dtype=torch.uint8, device="cuda", generator=g),
                             rs.randint(0, 4, 1500), rs.choice([-1.0, 0.0, 1.0], size=1500), rs.random_sample(1500) < 0.01)
        return agent, mem

    def run(agent, mem):
        g = torch.Generator(device="cuda").manual_seed(11)
        trace, pend = [], []
        for k in range(8):
            mem.priority_weight = min(1.0, 0.4 + 0.05 * k)
            agent.reset_noise()
            agent.learn(mem)
            pend.append(bool(agent._update_pending))
            trace.append(agent._loss.clone())
            if k in (2, 3):
                st = torch.rand(4, 84, 84, device="cuda", generator=g)
                trace.append(torch.tensor([float(agent.act(st)), agent.evaluate_q(st)], device="cuda"))
            if k == 4:
                agent.update_target_net()
            if k == 5:
                trace.append(agent.state_dict()["fc_h_v.weight_mu"].flatten()[:64].clone())
            if k == 6:
                trace.append(agent._norm.clone())
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in trace], pend

    a1, m1 = fresh("1")
    a2, m2 = fresh("0")
    assert a1._defer_update and not a2._defer_update
    assert a1._implicit_sigma and not a2._implicit_sigma
    t1, p1 = run(a1, m1)
    t2, p2 = run(a2, m2)
    assert all(p1) and not any(p2)
    assert len(t1) == len(t2)
    for i, (x, y) in enumerate(zip(t1, t2)):
        assert np.array_equal(x, y), i
    assert a1._update_pending                                        # ... and the accessors below run it
    assert torch.equal(a1.params.detach(), a2.params.detach()) and torch.equal(a1.target_params, a2.target_params)
    assert not a1._update_pending
    s1, s2 = a1.optimiser.state[a1.params], a2.optimiser.state[a2.params]
    assert torch.equal(s1["exp_avg"], s2["exp_avg"]) and torch.equal(s1["exp_avg_sq"], s2["exp_avg_sq"])
    assert torch.equal(a1.grads, a2.grads) and torch.equal(a1._norm, a2._norm)
    assert int(a1._step_dev.item()) == int(a2._step_dev.item()) == 8
    assert np.array_equal(m1._grab("tree"), m2._grab("tree"))



def test_checkpoint_restore_resumes_bit_exactly(hip, tmp_path):
    """SURVEY 8f row 3 'exact resume': run 6 steps, checkpoint agent + replay after step 3, restore both into FRESH
    objects and run steps 4-6 again: parameters, Adam moments, noise, per-sample losses and the sum-tree must come out
    bit-identical (device Philox streams of the noise generator and the sampler included)."""
    import io
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    args = _args(architecture="data-efficient", hidden_size=64, batch_size=16)
    env = types.SimpleNamespace(action_space=lambda: 4)

    def fresh():
        torch.manual_seed(77)
        np.random.seed(77)
        agent = Agent(args, env)
        mem = ReplayMemory(args, 2048, seed=5)
        g = torch.Generator(device="cuda").manual_seed(3)
        rs = np.random.RandomState(3)
        for _ in range(2):
            mem.append_batch(torch.randint(0, 256, (1500, 84, 84), dtype=torch.uint8, device="cuda", generator=g),
                             rs.randint(0, 4, 1500), rs.choice([-1.0, 0.0, 1.0], size=1500), rs.random_sample(1500) < 0.01)
        return agent, mem

    def run(agent, mem, steps):
        losses = []
        for k in steps:
            mem.priority_weight = min(1.0, 0.4 + 0.05 * k)
            agent.reset_noise()
            agent.learn(mem)
            losses.append(agent._loss.clone())
            if k == 4:
                agent.update_target_net()
        torch.cuda.synchronize()
        return torch.stack(losses).cpu().numpy()

    a1, m1 = fresh()
    run(a1, m1, range(3))
    ck = a1.checkpoint(str(tmp_path / "agent.ck"))
    buf = io.BytesIO()
    m1.save_to(buf, chunk_bytes=1 << 20)
    tail1 = run(a1, m1, range(3, 6))
    a2, _unused = fresh()
    a2.restore(str(tmp_path / "agent.ck"))
    buf.seek(0)
    m2 = ReplayMemory.load_from(buf, torch.device("cuda:0"), chunk_bytes=1 << 20)
    tail2 = run(a2, m2, range(3, 6))
    assert np.array_equal(tail1, tail2)
    assert torch.equal(a1.params.detach(), a2.params.detach()) and torch.equal(a1.target_params, a2.target_params)
    assert torch.equal(a1.noise, a2.noise) and torch.equal(a1.target_noise, a2.target_noise)
    s1, s2 = a1.optimiser.state[a1.params], a2.optimiser.state[a2.params]
    assert torch.equal(s1["exp_avg"], s2["exp_avg"]) and torch.equal(s1["exp_avg_sq"], s2["exp_avg_sq"])
    assert float(s1["step"]) == float(s2["step"]) == 6.0
    assert np.array_equal(m1._grab("tree"), m2._grab("tree"))
    assert bytes(m1._header()) == bytes(m2._header())
    assert isinstance(ck, dict) and ck["adam_step"] == 3.0


@pytest.mark.gpu
def test_one_call_step_equals_three_call_step(hip, monkeypatch):
    """Agent.learn's default path hands the whole step to rb_learner_train_step (one C call: sample + noise, learn, clip +
    Adam); RAINBOW_AMD_ONE_CALL=0 issues the same three entry points from Python.  Same launches, same arguments: after 8
    steps with beta annealing, a deferred online-noise draw and a target sync, parameters, moments, per-sample losses and
    the sum-tree must be bit-identical."""
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    args = _args(architecture="canonical", hidden_size=64, batch_size=16)
    env = types.SimpleNamespace(action_space=lambda: 4)

    def run(one_call):
        monkeypatch.setenv("RAINBOW_AMD_ONE_CALL", one_call)
        torch.manual_seed(11)
        np.random.seed(11)
        agent = Agent(args, env)
        assert agent._one_call == (one_call == "1")
        mem = ReplayMemory(args, 4096, seed=9)
        g = torch.Generator(device="cuda").manual_seed(4)
        rs = np.random.RandomState(4)
        for _ in range(3):
            mem.append_batch(torch.randint(0, 256, (1500, 84, 84), dtype=torch.uint8, device="cuda", generator=g),
                             rs.randint(0, 4, 1500), rs.choice([-1.0, 0.0, 1.0], size=1500), rs.random_sample(1500) < 0.01)
        losses = []
        for k in range(8):
            mem.priority_weight = min(1.0, 0.4 + 0.05 * k)
            if k % 2 == 0:
                agent.reset_noise()
            agent.learn(mem)
            losses.append(agent._loss.clone())
            if k == 4:
                agent.update_target_net()
        torch.cuda.synchronize()
        st = agent.optimiser.state[agent.params]
        return dict(params=agent.params.detach().cpu().numpy(), m=st["exp_avg"].cpu().numpy(), v=st["exp_avg_sq"].cpu().numpy(),
                    step=float(st["step"]), losses=torch.stack(losses).cpu().numpy(), total=mem._header().total,
                    idx=mem._buffers(16)["tree_idxs"].cpu().numpy(), used_one_call=agent._ts is not None)

    a, b = run("1"), run("0")
    assert a["used_one_call"] and not b["used_one_call"]
    assert a["step"] == b["step"] == 8.0
    for k in ("params", "m", "v", "losses", "idx"):
        assert np.array_equal(a[k], b[k]), k
    assert a["total"] == b["total"]


def test_update_target_net_copies_noise_buffers_too(hip):
    """agent.py:102-103: target.load_state_dict(online.state_dict()) carries the epsilon buffers (model.py:19,22) — after
    update_target_net the target's noise IS the online noise (until the next learn() redraws it, agent.py:74)."""
    from rainbow_amd.agent import Agent
    env = types.SimpleNamespace(action_space=lambda: 4)
    torch.manual_seed(5)
    agent = Agent(_args(), env)
    agent.reset_noise(torch.randn(int(agent.noise.numel())))          # injected online draw (materialised at once)
    agent._reset_target_noise()                                       # device RNG: a different target draw
    with torch.no_grad():
        agent.params.add_(0.5)
    torch.cuda.synchronize()
    assert not torch.equal(agent.target_noise, agent.noise) and not torch.equal(agent.target_params, agent.params.detach())
    agent.update_target_net()
    torch.cuda.synchronize()
    assert torch.equal(agent.target_noise, agent.noise) and float(agent.noise.abs().sum()) > 0
    assert torch.equal(agent.target_params, agent.params.detach())


def test_early_draw_random_interleaving_is_bit_identical(hip, monkeypatch):
    """RB_OPTS spec_draw=1 (opt-in) against a twin with spec_draw=0 through 240 randomly interleaved operations on the classes —
    runs of back-to-back learn() (where the early draw is launched and accepted), beta changes (a tentative draw rejected inside
    the sampler launch), appends / append_batch / update_priorities / sample / header reads (the replay's stream joined, the draw
    cancelled), act / evaluate_q / update_target_net / state_dict (which do not touch the replay: the streak goes on), and
    learn() with INJECTED target noise — the step's entry points one by one with the cached frame_source() window pointer
    (table 0): that draw must never accept the tentative one, which sits in the other table — : after
    every operation that returns something the two agents agree, and at the end parameters, moments, noise, the sum-tree, the
    frames' bookkeeping columns and the replay header (Philox counter included) are bit-identical."""
    from oracle import learner_oracle as O
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    args = _args(architecture="data-efficient", hidden_size=64, batch_size=16)
    env = types.SimpleNamespace(action_space=lambda: 4)

    def fresh(spec):
        monkeypatch.setenv("RB_OPTS", "implicit_small=1,spec_draw=%d" % spec)
        torch.manual_seed(91)
        np.random.seed(91)
        agent = Agent(args, env)
        mem = ReplayMemory(args, 2048, seed=7)
        g = torch.Generator(device="cuda").manual_seed(5)
        rs = np.random.RandomState(5)
        for _ in range(2):
            mem.append_batch(torch.randint(0, 256, (1500, 84, 84), dtype=torch.uint8, device="cuda", generator=g),
                             rs.randint(0, 4, 1500), rs.choice([-1.0, 0.0, 1.0], size=1500), rs.random_sample(1500) < 0.01)
        return agent, mem

    twins = [fresh(1), fresh(0)]
    rs = np.random.RandomState(123)
    g = torch.Generator(device="cuda").manual_seed(17)
    ops = ["learn"] * 10 + ["learn_injected"] * 2 + ["act", "evalq", "append", "append_batch", "beta", "target", "update", "sample", "header", "state_dict"]
    draws = O.noise_draw_count(O.Config(architecture="data-efficient", hidden=64, batch=16, actions=4, multi_step=args.multi_step,
                                        history=4, atoms=51, v_min=-10.0, v_max=10.0, discount=0.99))
    learns = 0
    injected_after_learn = 0
    prev = None
    for step in range(240):
        op = ops[rs.randint(len(ops))]
        st = torch.rand(4, 84, 84, device="cuda", generator=g)
        fr = torch.randint(0, 256, (5, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
        a_, r_, t_ = int(rs.randint(4)), float(rs.choice([-1.0, 0.0, 1.0])), bool(rs.random_sample() < 0.05)
        loss_ = torch.rand(16, device="cuda", generator=g) + 0.05
        # (leaf indices of its own: after learn() the speculating handle's sample buffers already hold the NEXT call's batch)
        idx_ = torch.from_numpy(np.sort(rs.randint(0, 2048, 16)) + 2047).cuda()
        beta_ = float(min(1.0, 0.4 + 0.002 * step))
        raw_ = rs.randn(draws).astype(np.float32)
        injected_after_learn += op == "learn_injected" and prev == "learn"
        prev = op
        outs = []
        for agent, mem in twins:
            if op == "learn":
                agent.reset_noise()
                agent.learn(mem)
                outs.append(agent._loss.clone())
            elif op == "learn_injected":
                agent.learn(mem, _target_raw_normals=torch.from_numpy(raw_))
                outs.append(agent._loss.clone())
            elif op == "act":
                outs.append(torch.tensor([agent.act(st)]))
            elif op == "evalq":
                outs.append(torch.tensor([agent.evaluate_q(st)]))
            elif op == "append":
                mem.append(st, a_, r_, t_)
            elif op == "append_batch":
                mem.append_batch(fr, [a_] * 5, [r_] * 5, [t_, False, False, False, False])
            elif op == "beta":
                mem.priority_weight = beta_
            elif op == "target":
                agent.update_target_net()
            elif op == "update":
                mem.update_priorities(idx_, loss_)
            elif op == "sample":
                o = mem.sample_device(16)
                outs.append(o["tree_idxs"].clone())
            elif op == "header":
                h = mem._header()
                outs.append(torch.tensor([h.index, h.full, h.last_attempts, h.last_status, h.rng_counter], dtype=torch.float64))
            elif op == "state_dict":
                outs.append(agent.state_dict()["fc_z_a.weight_mu"].flatten()[:32].clone())
        learns += op == "learn"
        if outs:
            torch.cuda.synchronize()
            assert torch.equal(outs[0].cpu(), outs[1].cpu()), (step, op)
    assert learns > 80 and injected_after_learn >= 5
    (a1, m1), (a2, m2) = twins
    assert m1.expired_waits() == 0 and m1.dropped_updates() == 0
    assert torch.equal(a1.params.detach(), a2.params.detach()) and torch.equal(a1.target_params, a2.target_params)
    s1, s2 = a1.optimiser.state[a1.params], a2.optimiser.state[a2.params]
    assert torch.equal(s1["exp_avg"], s2["exp_avg"]) and torch.equal(s1["exp_avg_sq"], s2["exp_avg_sq"])
    assert torch.equal(a1.noise, a2.noise) and torch.equal(a1.target_noise, a2.target_noise)
    d1, d2 = m1._dump(), m2._dump()
    for k in ("tree", "timestep", "action", "reward", "nonterminal"):
        assert np.array_equal(d1[k], d2[k]), k
    h1, h2 = m1._header(), m2._header()
    assert (h1.index, h1.full, h1.max, h1.total, h1.rng_counter) == (h2.index, h2.full, h2.max, h2.total, h2.rng_counter)
    assert m1.failed_samples() == m2.failed_samples() == 0


def test_expired_gate_of_the_early_draw_fails_safe(hip, monkeypatch):
    """(tests/ts_scenarios.py) on the device the gate really polls for ~2 ms before it gives up."""
    import ts_scenarios
    from cabi_adapter import TorchMem
    ts_scenarios.early_draw_expiry_check(hip, TorchMem, monkeypatch)


@pytest.mark.parametrize("preceding", [3, 4])
def test_public_sample_after_an_early_draw_reads_table_zero(hip, monkeypatch, preceding):
    """(tests/test_learner_emu.py, same name) on the device: two streams, the tentative draw really in flight."""
    import ts_scenarios
    from cabi_adapter import TorchMem
    ts_scenarios.public_sample_after_early_draw_check(hip, TorchMem, monkeypatch, preceding)


def test_train_step_captured_into_a_graph_with_the_early_draw_option(hip, monkeypatch):
    """(tests/ts_scenarios.py captured_train_step_check)"""
    import ts_scenarios
    from cabi_adapter import TorchMem
    ts_scenarios.captured_train_step_check(hip, TorchMem, monkeypatch)
