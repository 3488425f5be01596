"""S interleaved environment streams in one replay on the MI355X: the host-interpreter checks of test_replay_streams_emu.py
on the device, a 1M-slot 16-stream replay whose sampler is pinned to the oracle, a learn step drawn from an 8-stream replay
against the learner oracle, the vectorised acting loop (act_batch + append_streams + learn) and save / restore."""
import ctypes as C
import io
import pickle
import types

import numpy as np
import pytest
import torch

import streams_scenarios as SS
from cabi_adapter import TorchMem
from helpers import F32_ULP_RTOL, oracle_view_of_device_replay
from oracle import learner_oracle as O
from oracle.replay_oracle import tree_geometry
from streams_oracle import StreamsOracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib as L
    return L.load()


def _args(**kw):
    base = dict(device=torch.device("cuda:0"), history_length=4, discount=0.99, multi_step=3, priority_weight=0.4,
                priority_exponent=0.5, atoms=51, V_min=-10.0, V_max=10.0, batch_size=8, norm_clip=10.0, model=None,
                learning_rate=6.25e-5, adam_eps=1.5e-4, architecture="canonical", hidden_size=64, noisy_std=0.1)
    base.update(kw)
    return types.SimpleNamespace(**base)


# ------------------------------------------------------------------ the emulator's checks on the device
def test_one_stream_is_todays_replay_on_device(hip):
    SS.check_s1_identity(hip, TorchMem())


@pytest.mark.parametrize("S", [2, 7, 16, 64])
def test_append_rounds_equal_sequential_appends_on_device(hip, S):
    SS.check_append_rounds(hip, TorchMem(), S, seed=200 + S)


@pytest.mark.parametrize("n", [3, 20])
@pytest.mark.parametrize("S", [2, 16, 64])
def test_sampling_matches_the_restatement_on_device(hip, S, n):
    SS.check_sampling(hip, TorchMem(), S, n, seed=20 * S + n)


def test_draw_rejected_near_the_write_head_on_device(hip):
    SS.check_reject_near_head(hip, TorchMem())


@pytest.mark.parametrize("S", [3, 8])
def test_validation_states_follow_the_stream_on_device(hip, S):
    SS.check_states_at(hip, TorchMem(), S, seed=S)


def test_create_refuses_bad_stream_layouts_on_device(hip):
    SS.check_create_refusals(hip)


# ------------------------------------------------------------------ full size
def _round_timesteps(t0, terms):
    """Per-stream episode timesteps of R rounds ([R, S] terminal flags) starting from t0 [S]; returns (ts [R, S], t_next)."""
    ts = np.empty(terms.shape, dtype=np.int32)
    t = t0.copy()
    for r in range(terms.shape[0]):
        ts[r] = t
        t = np.where(terms[r], 0, t + 1).astype(np.int32)
    return ts, t


def _streams_view(mem, beta):
    """StreamsOracle over the device's own tree and columns (no frame store): what oracle_view_of_device_replay is for S = 1."""
    base = oracle_view_of_device_replay(mem, beta=beta)
    ora = StreamsOracle.__new__(StreamsOracle)
    ora.__dict__.update(base.__dict__)
    ora.streams, ora.per_stream, ora.stream_t = mem.streams, None, mem.stream_t.copy()
    return ora


def test_sampler_indices_match_oracle_at_1m_with_16_streams(hip):
    """A 1M-slot replay of 16 streams (filled by whole rounds, then 200 rounds through rb_replay_append_streams on the 20-level
    tree): every internal node fl32(left + right); with injected uniforms the sampler's tree indices, attempts, window table,
    actions, returns, nonterminals (exact) and weights (4 ulp) against the restatement; pixels of a few stacks."""
    from rainbow_amd import _lib as L
    from rainbow_amd.memory import ReplayMemory
    S, cap, chunk = 16, 1_000_000, 50_000
    mem = ReplayMemory(_args(), cap, seed=6, streams=S)
    rs = np.random.RandomState(16)
    g = torch.Generator(device="cuda").manual_seed(16)
    t = np.zeros(S, dtype=np.int32)
    for lo in range(0, cap + chunk, chunk):
        R = chunk // S
        terms = rs.random_sample((R, S)) < 2e-3
        ts, t = _round_timesteps(t, terms)
        fr = torch.randint(0, 256, (chunk, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
        cols = [torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda() for x in
                (ts, rs.randint(0, 6, (R, S)).astype(np.int32), rs.choice([-1.0, 0.0, 1.0], size=(R, S)).astype(np.float32),
                 (~terms).astype(np.uint8))]
        L.check(hip, hip.rb_replay_append_batch(mem._h, fr.data_ptr(), *[c.data_ptr() for c in cols], chunk, mem._stream()))
        torch.cuda.synchronize()
    mem.stream_t = t
    levels, tree_start, tree_len = tree_geometry(cap)
    for r in range(40):
        idx = torch.randint(0, cap, (1024,), device="cuda", generator=g) + tree_start
        mem.update_priorities(idx, torch.rand(1024, device="cuda", generator=g) * 3 + 1e-3)
    states = torch.rand((S, 4, 84, 84), device="cuda", generator=g)
    for r in range(200):
        mem.append_streams(states, rs.randint(0, 6, S), rs.choice([-1.0, 0.0, 1.0], size=S), rs.random_sample(S) < 0.01)
    torch.cuda.synchronize()
    hdr = mem._header()
    assert hdr.full == 1 and hdr.index == (chunk + 200 * S) % cap and mem.transitions.index == hdr.index
    tree = mem._grab("tree")
    p = np.arange(0, tree_start)
    p = p[2 * p + 2 < tree_len]
    assert np.array_equal(tree[p], tree[2 * p + 1] + tree[2 * p + 2])
    assert hdr.total == tree[0]
    ora = _streams_view(mem, beta=0.6)
    mem.priority_weight = 0.6
    for B in (32, 256):
        for rep in range(3):
            uu = rs.random_sample((32, B))
            o = mem.sample_device(B, torch.from_numpy(uu))
            torch.cuda.synchronize()
            assert mem._header().last_status == 0
            probs, idxs, tree_idxs, attempts = ora.draw_indices(B, uu)
            assert np.array_equal(o["tree_idxs"].cpu().numpy(), tree_idxs), (B, rep)
            assert mem._header().last_attempts == attempts
            sc = ora.batch_scalars(idxs, probs)
            assert np.array_equal(o["actions"].cpu().numpy(), sc["actions"])
            assert np.array_equal(o["returns"].cpu().numpy(), sc["returns"])
            assert np.array_equal(o["nonterminals"].cpu().numpy(), sc["nonterminals"][:, 0])
            np.testing.assert_allclose(o["weights"].cpu().numpy(), sc["weights"], rtol=F32_ULP_RTOL)
            _, win_ptr, wl = mem.frame_source()
            win = np.empty((B, wl), dtype=np.int32)
            L.check(hip, hip.rb_copy_to_host(win.ctypes.data, win_ptr, win.nbytes, mem._stream()))
            assert np.array_equal(win, np.where(sc["blank"], -1, sc["ring"]))
            s, ns = o["states"].cpu().numpy(), o["next_states"].cpu().numpy()
            for b in (0, B - 1):
                for k in range(4):
                    for arr, slot in ((s, k), (ns, 3 + k)):
                        want = (np.zeros((84, 84), np.uint8) if sc["blank"][b, slot]
                                else mem._grab("frames", int(sc["ring"][b, slot]), 1)[0])
                        assert np.array_equal(arr[b, k], want), (B, b, k)
    del mem
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ the learner on an S-stream batch
def _synthetic_round(rs, S, A):
    st = (rs.randint(0, 256, size=(S, 4, 84, 84)).astype(np.float32) / np.float32(255)).astype(np.float32)
    return st, rs.randint(0, A, S), rs.choice([-1.0, 0.0, 1.0], size=S).astype(np.float32), rs.random_sample(S) < 0.03


def test_learn_step_from_an_8_stream_replay_matches_the_learner_oracle(hip):
    """Agent.learn on an 8-stream replay (the zero-copy conv path reads the ring through the sampler's window table, which
    carries the stream stride) against the oracle sample of the restatement + the learner oracle: tree indices exact,
    loss, norm, post-Adam parameters within the tolerances of tests/helpers.py."""
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    S, cap, A = 8, 8 * 256, 6
    args = _args()
    B = args.batch_size
    torch.manual_seed(4)
    agent = Agent(args, types.SimpleNamespace(action_space=lambda: A))
    mem = ReplayMemory(args, cap, seed=12, streams=S)
    ora = StreamsOracle(cap, S, per_stream=False)
    rs = np.random.RandomState(31)
    for r in range(300):
        st, a, rw, te = _synthetic_round(rs, S, A)
        mem.append_streams(torch.from_numpy(st).cuda(), a, rw, te)
        ora.append_round(st, a, rw, te)
    cfg = O.Config(batch=B, atoms=51, actions=A, history=4, hidden=args.hidden_size, architecture="canonical", multi_step=3)
    online = {k: v.cpu().numpy() for k, v in agent.state_dict().items() if "epsilon" not in k}
    target = {k: v.copy() for k, v in online.items()}
    adam = O.AdamOracle(online, args.learning_rate, args.adam_eps)
    draws = O.noise_draw_count(cfg)
    for step in range(3):
        raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
        uu = rs.random_sample((32, B))
        agent.reset_noise(torch.from_numpy(raw_on))
        agent.learn(mem, _target_raw_normals=torch.from_numpy(raw_tg), _unit_uniforms=torch.from_numpy(uu))
        batch = ora.sample_with_uniforms(B, uu)
        want = O.learn(cfg, online, target, O.make_noise(cfg, raw_on), O.make_noise(cfg, raw_tg), batch)
        total, clipped = O.clip_grads(want["grads"], args.norm_clip)
        online = adam.step(clipped)
        ora.update_priorities(batch["tree_idxs"], want["loss"])
        torch.cuda.synchronize()
        assert np.array_equal(mem._out[B]["tree_idxs"].cpu().numpy(), batch["tree_idxs"]), step
        np.testing.assert_allclose(agent._loss.cpu().numpy(), want["loss"], rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(float(agent._norm.item()), total, rtol=5e-5, atol=1e-7)
        got = {k: v.cpu().numpy() for k, v in agent.state_dict().items() if "epsilon" not in k}
        for k in online:
            np.testing.assert_allclose(got[k], online[k], rtol=0, atol=2e-7, err_msg="step %d %s" % (step, k))
        # one more round between learn calls: the write head moves under the sampler
        st, a, rw, te = _synthetic_round(rs, S, A)
        mem.append_streams(torch.from_numpy(st).cuda(), a, rw, te)
        ora.append_round(st, a, rw, te)


def test_vectorised_loop_keeps_the_tree_exact(hip):
    """500 rounds of the vectorised actor loop at S = 16 (act_batch on the 16 frame stacks, append_streams, and one learn per
    replay_frequency = 4 environment steps, i.e. 4 per round, once 64 rounds are in): afterwards every internal node is
    fl32(left + right) of its children, header total == root and the loss is finite."""
    from rainbow_amd.agent import Agent
    from rainbow_amd.memory import ReplayMemory
    S, A, cap = 16, 6, 16 * 1024
    args = _args()
    torch.manual_seed(5)
    agent = Agent(args, types.SimpleNamespace(action_space=lambda: A))
    mem = ReplayMemory(args, cap, seed=13, streams=S)
    g = torch.Generator(device="cuda").manual_seed(5)
    rs = np.random.RandomState(5)
    stacks = torch.zeros((S, 4, 84, 84), device="cuda")
    learns = 0
    for r in range(500):
        frame = torch.rand((S, 84, 84), device="cuda", generator=g)
        stacks = torch.cat([stacks[:, 1:], frame[:, None]], dim=1)
        actions = agent.act_batch(stacks)
        assert actions.shape == (S,) and np.all((actions >= 0) & (actions < A))
        terms = rs.random_sample(S) < 0.01
        mem.append_streams(stacks, actions, rs.choice([-1.0, 0.0, 1.0], size=S), terms)
        if terms.any():
            stacks[torch.from_numpy(terms).cuda()] = 0.0
        if r >= 64:
            for _ in range(S // 4):
                agent.reset_noise()
                agent.learn(mem)
                learns += 1
    torch.cuda.synchronize()
    assert learns == 436 * 4 and mem.failed_samples() == 0
    assert np.all(np.isfinite(agent._loss.cpu().numpy()))
    levels, tree_start, tree_len = tree_geometry(cap)
    tree = mem._grab("tree")
    p = np.arange(0, tree_start)
    p = p[2 * p + 2 < tree_len]
    assert np.array_equal(tree[p], tree[2 * p + 1] + tree[2 * p + 2])
    hdr = mem._header()
    assert hdr.total == tree[0] and hdr.index == (500 * S) % cap and hdr.full == 0


# ------------------------------------------------------------------ save / restore
def test_save_load_and_pickle_keep_streams(hip):
    """save_to / load_from and pickle at S = 8 carry S and the per-stream timesteps; the restored replay gives the identical
    next sample (injected uniforms) and keeps appending rounds identically."""
    from rainbow_amd.memory import ReplayMemory
    S, cap = 8, 8 * 64
    mem = ReplayMemory(_args(), cap, seed=3, streams=S)
    rs = np.random.RandomState(8)
    for r in range(100):
        st, a, rw, te = _synthetic_round(rs, S, 6)
        mem.append_streams(torch.from_numpy(st).cuda(), a, rw, te)
    o = mem.sample_device(8)
    mem.update_priorities(o["tree_idxs"], torch.rand(8, device="cuda") + 0.1)
    buf = io.BytesIO()
    mem.save_to(buf)
    buf.seek(0)
    loaded = ReplayMemory.load_from(buf, torch.device("cuda:0"))
    unpickled = pickle.loads(pickle.dumps(mem))
    with pytest.raises(RuntimeError, match="append_streams"):
        mem.append(torch.zeros(4, 84, 84, device="cuda"), 0, 0.0, False)
    with pytest.raises(RuntimeError, match="append_streams"):
        mem.append_batch(torch.zeros(8, 84, 84, dtype=torch.uint8, device="cuda"), [0] * 8, [0.0] * 8, [False] * 8)
    st, a, rw, te = _synthetic_round(rs, S, 6)
    uu = np.random.RandomState(9).random_sample((32, 16))
    ref = None
    saved_t = mem.stream_t.copy()
    assert np.any(saved_t != saved_t[0])            # the streams are at different points of their episodes
    for m in (mem, loaded, unpickled):
        assert m.streams == S and np.array_equal(m.stream_t, saved_t)
        s = C.c_int32(0)
        hip.rb_replay_streams(m._h, C.byref(s))
        assert s.value == S
        x = m.sample_device(16, torch.from_numpy(uu))["tree_idxs"].cpu().numpy()
        m.append_streams(torch.from_numpy(st).cuda(), a, rw, te)
        d = m._dump()
        got = (x, d, m.stream_t.copy())
        if ref is None:
            ref = got
            continue
        assert np.array_equal(got[0], ref[0])
        for k in d:
            assert np.array_equal(np.frombuffer(d[k], np.uint8) if isinstance(d[k], bytes) else d[k],
                                  np.frombuffer(ref[1][k], np.uint8) if isinstance(ref[1][k], bytes) else ref[1][k]), k
        assert np.array_equal(got[2], ref[2])
