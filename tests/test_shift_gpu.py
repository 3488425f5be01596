"""Random-shift augmentation in the replay's frame-stack gather on the MI355X: the checks of tests/shift_scenarios.py against
librainbow_hip.so (k_gather_stacks_shift, csrc/replay_shift.h), then the drop-in classes — ReplayMemory(augment_pad=...) and
Agent.learn on it — against tests/shift_oracle.py and the oracle replay / learner.  Stacks and shifts compare exactly."""
import io
import pickle
import types

import numpy as np
import pytest
import torch

import shift_oracle as SO
import shift_scenarios as SH
from cabi_adapter import TorchMem
from guarded_mem import GuardedTorchMem
from oracle import learner_oracle as O
from oracle.replay_oracle import ReplayOracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib as L
    return L.load()


@pytest.mark.parametrize("pad", [1, 4, 8])
@pytest.mark.parametrize("history,n,streams", [(4, 3, 1), (1, 1, 1), (3, 20, 1), (4, 3, 3)],
                         ids=["h4-n3", "h1-n1", "h3-n20", "h4-n3-3streams"])
def test_every_shift_matches_the_oracle_on_device(hip, history, n, streams, pad):
    SH.check_injected_enumeration(hip, TorchMem(), history, n, pad, streams=streams)


def test_pad_zero_is_the_plain_gather_on_device(hip):
    SH.check_pad_zero_is_the_plain_gather(hip, TorchMem())


@pytest.mark.parametrize("seed", [7, 0x9E3779B97F4A7C15])
def test_device_draws_match_the_oracle_and_leave_the_header_alone_on_device(hip, seed):
    SH.check_philox_path(hip, TorchMem(), seed)


def test_gather_stays_inside_the_callers_buffers_on_device(hip):
    SH.check_guard_bands(hip, GuardedTorchMem())


def test_refusals_name_the_argument_and_launch_nothing_on_device(hip):
    SH.check_refusals(hip, TorchMem())


def test_learn_step_on_shifted_stacks_matches_the_oracle_on_device(hip):
    SH.check_learn_step(hip, TorchMem())


# =============================================================================== the classes
def _args(**kw):
    base = dict(device=torch.device("cuda:0"), history_length=4, discount=0.99, multi_step=3, priority_weight=0.4,
                priority_exponent=0.5, atoms=51, V_min=-10.0, V_max=10.0, batch_size=8, norm_clip=10.0, model=None,
                learning_rate=6.25e-5, adam_eps=1.5e-4, architecture="data-efficient", hidden_size=64, noisy_std=0.1)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _transitions(total, actions, seed):
    rs = np.random.RandomState(seed)
    frames = np.stack([SH.frame_of(k) for k in range(total)])
    return frames, rs.randint(0, actions, total), rs.choice([-1.0, 0.0, 1.0], size=total).astype(np.float32), rs.random_sample(total) < 0.12


def _filled(args, cap, total, seed, actions=3):
    from rainbow_amd.memory import ReplayMemory
    mem = ReplayMemory(args, cap, seed=seed)
    fr, ac, rw, te = _transitions(total, actions, 5)
    for lo in range(0, total, cap // 2):
        hi = min(total, lo + cap // 2)
        mem.append_batch(torch.from_numpy(fr[lo:hi]).cuda(), ac[lo:hi], rw[lo:hi], te[lo:hi])
    return mem


def _host(o):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in o.items()}


def test_replay_memory_option_shifts_sampled_stacks_only(hip):
    """ReplayMemory(augment_pad=4) against a twin without the option (same seed, same appends): the same draw, the stacks the
    oracle's shift of the twin's under o["shifts"], o["shifts"] the oracle's draw number 0, 1, 2, ...; the draw number and the pad
    travel through pickling and save_to / load_from; sample() is shifted, states_at is not."""
    from rainbow_amd.memory import ReplayMemory
    seed, cap, total, B, pad = 23, 256, 300, 5, 4
    twin = _filled(_args(), cap, total, seed)
    aug = _filled(_args(augment_pad=pad), cap, total, seed)
    assert aug.augment_pad == pad and twin.augment_pad == 0
    rs = np.random.RandomState(9)
    saw_blank = False
    for draw in (0, 1):
        uu = torch.from_numpy(rs.random_sample((16, B)))
        want, got = _host(twin.sample_device(B, unit_uniforms=uu)), _host(aug.sample_device(B, unit_uniforms=uu))
        assert "shifts" not in want and got["shifts"].dtype == np.int8 and got["shifts"].shape == (B, 2, 2)
        for k in ("tree_idxs", "actions", "returns", "nonterminals", "weights"):
            assert np.array_equal(want[k], got[k]), (draw, k)
        assert np.array_equal(got["shifts"], SO.draw_shifts(seed, draw, B, pad)), draw
        ws, wn = SO.shift_batch(want["states"], want["next_states"], got["shifts"])
        assert np.array_equal(got["states"], ws) and np.array_equal(got["next_states"], wn), draw
        assert not np.array_equal(got["states"], want["states"])
        saw_blank |= bool((want["states"].reshape(B, 4, -1).max(axis=2) == 0).any())
    assert saw_blank, "the scenario must contain a blanked frame"
    assert aug._aug_draw == 2
    # injected shifts through the class, gather=False untouched by the option
    inj = np.array([[[4, -4], [-4, 4]]] * B, dtype=np.int8)
    uu = torch.from_numpy(rs.random_sample((16, B)))
    want, got = _host(twin.sample_device(B, unit_uniforms=uu)), _host(aug.sample_device(B, unit_uniforms=uu, shifts=torch.from_numpy(inj)))
    ws, wn = SO.shift_batch(want["states"], want["next_states"], inj)
    assert np.array_equal(got["shifts"], inj) and np.array_equal(got["states"], ws) and np.array_equal(got["next_states"], wn)
    before = aug._aug_draw
    aug.sample_device(B, unit_uniforms=uu, gather=False)
    assert aug._aug_draw == before == 3
    # pickle and save_to / load_from carry the pad and the draw number: the next batch is byte-identical
    blob = pickle.dumps(aug)
    stream = io.BytesIO()
    aug.save_to(stream)
    stream.seek(0)
    uu = torch.from_numpy(rs.random_sample((16, B)))
    nxt = _host(aug.sample_device(B, unit_uniforms=uu))
    assert np.array_equal(nxt["shifts"], SO.draw_shifts(seed, 3, B, pad))
    for restored in (pickle.loads(blob), ReplayMemory.load_from(stream, "cuda:0")):
        assert restored.augment_pad == pad and restored._aug_draw == 3
        again = _host(restored.sample_device(B, unit_uniforms=uu))
        for k in nxt:
            assert np.array_equal(nxt[k], again[k]), k
    # a state written before the option existed: off, draw 0
    st = aug.__getstate__()
    st.pop("augment_pad"); st.pop("_aug_draw")
    old = ReplayMemory.__new__(ReplayMemory)
    old.__setstate__(st)
    assert old.augment_pad == 0 and old._aug_draw == 0 and "shifts" not in old.sample_device(B, unit_uniforms=uu)
    # sample(): the reference's 7-tuple holds the shifted stacks / 255 (device RNG: both memories have drawn no device uniforms yet)
    t_twin, t_aug = twin.sample(B), aug.sample(B)
    torch.cuda.synchronize()
    assert np.array_equal(t_twin[0], t_aug[0])
    sh = aug._out[B]["shifts"].cpu().numpy()
    assert np.array_equal(sh, SO.draw_shifts(seed, 4, B, pad))
    u8 = [(t_twin[k].cpu().numpy() * 255).round().astype(np.uint8) for k in (1, 4)]
    ws, wn = SO.shift_batch(u8[0], u8[1], sh)
    assert torch.equal(t_aug[1].cpu(), torch.from_numpy(ws).float() / 255) and torch.equal(t_aug[4].cpu(), torch.from_numpy(wn).float() / 255)
    assert torch.equal(t_aug[1].cpu(), aug._out[B]["states"].cpu().float() / 255)      # (on the host: a correctly rounded division)
    # the validation view is never shifted
    idx = [0, 1, 17, cap - 1]
    assert torch.equal(aug.states_at(idx), twin.states_at(idx)) and bool(aug.states_at(idx).any())
    aug.current_idx = twin.current_idx = 17
    assert torch.equal(next(aug), next(twin))
    for bad in (-1, 9):
        with pytest.raises(ValueError, match="augment_pad"):
            ReplayMemory(_args(augment_pad=bad), cap, seed=seed)


def test_agent_learns_on_shifted_stacks_vs_oracle(hip):
    """Two Agent.learn(mem) calls on a ReplayMemory with augment_pad = 4 — the gathered path: the sampler launch hosting the noise
    job and (second call) the first call's deferred clip + Adam pass, the shifted gather, rb_learner_learn, the fused priority
    write-back — with injected sampler uniforms and noise, against the oracle replay + oracle learner fed the oracle-shifted stacks
    under the predicted shifts of draws 0 and 1.  Tolerances: those of test_learner_gpu.py's class-level tests at batch <= 32."""
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    seed, cap, total, pad, A, hidden = 29, 1024, 1500, 4, 3, 64
    args = _args(augment_pad=pad, hidden_size=hidden)
    B = args.batch_size
    env = types.SimpleNamespace(action_space=lambda: A)
    torch.manual_seed(4)
    agent = Agent(args, env)
    assert agent._defer_update and agent._fuse_update
    mem = _filled(args, cap, total, seed, actions=A)
    ora_mem = ReplayOracle(cap)
    fr, ac, rw, te = _transitions(total, A, 5)
    for i in range(total):
        ora_mem.append_frame(fr[i], int(ac[i]), float(rw[i]), bool(te[i]))
    cfg = O.Config(batch=B, atoms=51, actions=A, history=4, hidden=hidden, architecture="data-efficient", multi_step=3)
    online = {k: v.cpu().numpy() for k, v in agent.state_dict().items() if "epsilon" not in k}
    target = {k: v.copy() for k, v in online.items()}
    adam = O.AdamOracle(online, args.learning_rate, args.adam_eps)
    draws = O.noise_draw_count(cfg)
    rs = np.random.RandomState(31)
    want = []
    for step in range(2):
        raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
        uu = rs.random_sample((32, B))
        agent.reset_noise(torch.from_numpy(raw_on))
        was_pending = agent._update_pending
        agent.learn(mem, _target_raw_normals=torch.from_numpy(raw_tg), _unit_uniforms=torch.from_numpy(uu))
        assert agent._lib.rb_learner_priority_written(agent._h) == 1, "the priority write-back was not fused"
        batch = ora_mem.sample_with_uniforms(B, uu)
        shifts = SO.draw_shifts(seed, step, B, pad)
        batch["states"], batch["next_states"] = SO.shift_batch(batch["states"], batch["next_states"], shifts)
        out = O.learn(cfg, online, target, O.make_noise(cfg, raw_on), O.make_noise(cfg, raw_tg), batch)
        total_norm, clipped = O.clip_grads(out["grads"], args.norm_clip)
        online = adam.step(clipped)
        ora_mem.update_priorities(batch["tree_idxs"], out["loss"])
        want.append(dict(params={k: v.copy() for k, v in online.items()}, norm=total_norm))
        torch.cuda.synchronize()
        o = mem._out[B]
        assert np.array_equal(o["tree_idxs"].cpu().numpy(), batch["tree_idxs"]), step
        assert np.array_equal(o["shifts"].cpu().numpy(), shifts), step
        assert np.array_equal(o["states"].cpu().numpy(), batch["states"]) and np.array_equal(o["next_states"].cpu().numpy(), batch["next_states"])
        np.testing.assert_allclose(agent._loss.cpu().numpy(), out["loss"], rtol=2e-5, atol=1e-6, err_msg="step %d" % step)
        assert agent._update_pending, "the optimiser pass of step %d was not deferred" % step
        if was_pending:      # step 0's pass was hosted by this call's sampler launch: the parameters raw, no flush
            got = {name: agent._view(agent._params, name).cpu().numpy() for name, _o, _s in agent._layout}
            for k in want[0]["params"]:
                np.testing.assert_allclose(got[k], want[0]["params"][k], rtol=0, atol=3e-7, err_msg="hosted pass of step 0: %s" % k)
            np.testing.assert_allclose(float(agent._norm_buf.item()), want[0]["norm"], rtol=5e-5)
    assert was_pending and mem._aug_draw == 2
    got = {k: v.cpu().numpy() for k, v in agent.state_dict().items() if "epsilon" not in k}      # (flushes the last pass)
    for k in got:
        np.testing.assert_allclose(got[k], want[1]["params"][k], rtol=0, atol=3e-7, err_msg="final %s" % k)
    np.testing.assert_allclose(float(agent._norm.item()), want[1]["norm"], rtol=5e-5)
    np.testing.assert_allclose(mem._dump()["tree"], ora_mem.transitions.tree, rtol=2e-5)
