"""Checks of the S-stream replay (rb_replay_create_streams) shared by the host-interpreter tests
(test_replay_streams_emu.py) and the device tests (test_replay_streams_gpu.py): the same adapter drives either
build through the C ABI, tests/streams_oracle.py is the oracle."""
import ctypes as C

import numpy as np

from cabi_adapter import CAbiReplayAdapter
from helpers import F32_ULP_RTOL
from rainbow_amd import _lib as L
from streams_oracle import StreamsOracle


class StreamsAdapter(CAbiReplayAdapter):
    """CAbiReplayAdapter over rb_replay_create_streams, plus the round append and the raw columns."""

    def __init__(self, lib, mem, capacity, history, n, streams, discount=0.99, omega=0.5, seed=7):
        self.lib, self.mem = lib, mem
        self.capacity, self.history, self.n, self.streams = capacity, history, n, streams
        self.h = C.c_void_p()
        L.check(lib, lib.rb_replay_create_streams(C.byref(self.h), capacity, history, n, discount, omega, seed, streams))
        self.t = 0
        self.bufs = L.ReplayBuffers()
        L.check(lib, lib.rb_replay_buffers(self.h, C.byref(self.bufs)))
        self.stream_t = np.zeros(streams, dtype=np.int32)

    def append_round(self, states, actions, rewards, terminals):
        m = self.mem
        st = m.upload(np.asarray(states, dtype=np.float32))
        terminals = np.asarray(terminals, dtype=bool)
        ac = np.asarray(actions, dtype=np.int32)
        rw = np.asarray(rewards, dtype=np.float32)
        nt = (~terminals).astype(np.uint8)
        ts = self.stream_t.copy()
        L.check(self.lib, self.lib.rb_replay_append_streams(self.h, m.ptr(st), ts.ctypes.data, ac.ctypes.data, rw.ctypes.data,
                                                            nt.ctypes.data, m.stream))
        ts[:] = -1                    # the host arrays are free again once the call returns (by-value arguments)
        m.sync()
        self.stream_t = np.where(terminals, 0, self.stream_t + 1).astype(np.int32)

    def columns(self):
        m, b, cap = self.mem, self.bufs, self.capacity
        return dict(frames=m.view(b.frames_dev, (cap, 84, 84), np.uint8), timestep=m.view(b.timestep_dev, (cap,), np.int32),
                    action=m.view(b.action_dev, (cap,), np.int32), reward=m.view(b.reward_dev, (cap,), np.float32),
                    nonterminal=m.view(b.nonterminal_dev, (cap,), np.uint8))

    def windows(self, batch):
        return self.mem.view(self.bufs.window_dev, (batch, self.history + self.n), np.int32)

    def states_at(self, indices):
        m = self.mem
        idx = m.upload(np.asarray(indices, dtype=np.int64))
        out = m.empty((len(indices), self.history, 84, 84), np.float32)
        L.check(self.lib, self.lib.rb_replay_states_at(self.h, m.ptr(idx), len(indices), m.ptr(out), m.stream))
        m.sync()
        return m.download(out)


def episode_ends(rs, S, p):
    """Terminal flags of one round, staggered per stream (each stream its own episode lengths)."""
    return rs.random_sample(S) < p


def fill(ad, ora, rounds, rs, p_term=0.15, updates=True):
    """`rounds` append rounds into the adapter and the oracle; now and then a priority write-back so the running max moves."""
    S, h = ad.streams, ad.history
    tree_start = ora.transitions.tree_start
    for r in range(rounds):
        states = rs.random_sample((S, h, 84, 84)).astype(np.float32)      # arbitrary floats: x * 255 truncation
        if r % 3 == 0:
            states = (rs.randint(0, 256, size=(S, h, 84, 84)).astype(np.float32) / np.float32(255)).astype(np.float32)
        actions = rs.randint(0, 6, S)
        rewards = rs.choice([-1.0, 0.0, 0.5, 1.0], size=S).astype(np.float32)
        terms = episode_ends(rs, S, p_term)
        ad.append_round(states, actions, rewards, terms)
        ora.append_round(states, actions, rewards, terms)
        if updates and r % 7 == 3:
            k = min(64, ad.capacity)
            idx = rs.randint(0, ad.capacity, k) + tree_start
            vals = (rs.random_sample(k) * 3 + 0.05).astype(np.float32)
            ad.update_leaves(idx, vals)
            ora.transitions.set_leaves(idx, vals)
    assert np.array_equal(ad.stream_t, ora.stream_t)


def assert_same_replay(ad, ora, label=""):
    tr = ora.transitions
    col = ad.columns()
    assert np.array_equal(col["frames"], tr.frames), label
    assert np.array_equal(col["timestep"], tr.timestep), label
    assert np.array_equal(col["action"], tr.action), label
    assert np.array_equal(col["reward"], tr.reward), label
    assert np.array_equal(col["nonterminal"].astype(bool), tr.nonterminal), label
    assert np.array_equal(ad.tree(), tr.tree), label
    hdr = ad.raw_header()
    assert (int(hdr.index), bool(hdr.full)) == (tr.index, tr.full), label
    assert np.float32(hdr.max) == tr.max and np.float32(hdr.total) == tr.total(), label
    idx, full = C.c_int64(-1), C.c_int32(-1)
    L.check(ad.lib, ad.lib.rb_replay_position(ad.h, C.byref(idx), C.byref(full)))
    assert (idx.value, bool(full.value)) == (tr.index, tr.full), label


def check_s1_identity(lib, mem, capacity=256, rounds=400, seed=5):
    """rb_replay_create_streams(..., 1) + rb_replay_append_streams == rb_replay_create + rb_replay_append: ring, tree, header
    and a sampled batch with injected uniforms."""
    rs = np.random.RandomState(seed)
    one = StreamsAdapter(lib, mem, capacity, 4, 3, 1)
    ref = CAbiReplayAdapter(lib, mem, capacity, 4, 3, 0.99, 0.5)
    s = C.c_int32(0)
    L.check(lib, lib.rb_replay_streams(one.h, C.byref(s)))
    assert s.value == 1
    for r in range(rounds):
        st = rs.random_sample((1, 4, 84, 84)).astype(np.float32)
        a, rw, term = int(rs.randint(0, 6)), float(rs.choice([-1.0, 0.0, 1.0])), bool(rs.random_sample() < 0.05)
        one.append_round(st, [a], [rw], [term])
        ref.append(st[0], a, rw, term)
        if r % 50 == 49:
            idx = rs.randint(0, capacity, 16) + capacity - 1
            vals = (rs.random_sample(16) * 2 + 0.1).astype(np.float32)
            one.update_leaves(idx, vals)
            ref.update_leaves(idx, vals)
    c1, c2 = one.columns(), StreamsAdapter.columns(ref)
    for k in c1:
        assert np.array_equal(c1[k], c2[k]), k
    assert np.array_equal(one.tree(), ref.tree())
    fields = [f for f, _ in L.ReplayHeader._fields_]       # (field by field: the struct's padding bytes are never written)
    h1, h2 = one.raw_header(), ref.raw_header()
    assert [getattr(h1, f) for f in fields] == [getattr(h2, f) for f in fields]
    uu = rs.random_sample((64, 32))
    x, y = one.sample(32, uu, 0.5), ref.sample(32, uu, 0.5)
    for k in x:
        assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k
    assert np.array_equal(one.windows(32), StreamsAdapter.windows(ref, 32))
    one.close(); ref.close()


def check_append_rounds(lib, mem, S, seed, history=4, n=3):
    """Append rounds at a capacity the rounds wrap more than twice, episode ends staggered per stream, priority write-backs in
    between: ring, tree, max, total, index and full bit-exact against S * R sequential oracle appends, after EVERY few rounds."""
    Cs = 2 * (history + n) + 2
    cap = S * Cs
    rs = np.random.RandomState(seed)
    ad = StreamsAdapter(lib, mem, cap, history, n, S)
    ora = StreamsOracle(cap, S, history=history, multi_step=n, per_stream=False)
    for chunk in range(5):            # 5 * (Cs // 2 + 1) rounds: the ring wraps twice and stops mid-way
        fill(ad, ora, Cs // 2 + 1, rs)
        assert_same_replay(ad, ora, "S=%d chunk %d" % (S, chunk))
    assert ora.transitions.full and 5 * (Cs // 2 + 1) > 2 * Cs
    ad.close()


def make_sampling_replay(lib, mem, S, n, seed, history=4, Cs=48, zone_prob=1e-6):
    """A filled S-stream replay (ring wrapped, write head mid-ring) with random priorities, and tiny ones on the slots the
    validity rule excludes around the write head (so that batches of 256 find a valid draw within a few attempts)."""
    rs = np.random.RandomState(seed)
    cap = S * Cs
    ad = StreamsAdapter(lib, mem, cap, history, n, S)
    ora = StreamsOracle(cap, S, history=history, multi_step=n)
    fill(ad, ora, Cs + Cs // 2 + 3, rs, p_term=0.06, updates=False)
    tree_start = ora.transitions.tree_start
    for lo in range(0, cap, 1024):
        idx = np.arange(lo, min(cap, lo + 1024)) + tree_start
        vals = (rs.random_sample(len(idx)) * 2 + 0.25).astype(np.float32)
        ad.update_leaves(idx, vals)
        ora.transitions.set_leaves(idx, vals)
    head = ora.transitions.index
    zone = (head + np.arange(-(n + 1) * S, history * S)) % cap
    zone_vals = np.full(len(zone), zone_prob, dtype=np.float32)
    for lo in range(0, len(zone), 1024):
        ad.update_leaves(zone[lo:lo + 1024] + tree_start, zone_vals[lo:lo + 1024])
        ora.transitions.set_leaves(zone[lo:lo + 1024] + tree_start, zone_vals[lo:lo + 1024])
    assert np.array_equal(ad.tree(), ora.transitions.tree)
    return ad, ora, rs


def check_batch(ad, ora, B, uu, beta):
    """One draw with injected uniforms: everything exact against the restatement (weights 4 ulp), and every window equal to
    the single-stream oracle of its stream."""
    got = ad.sample(B, uu, beta)
    ora.priority_weight = beta
    want = ora.sample_with_uniforms(B, uu)
    assert got["attempts"] == want["attempts"]
    assert np.array_equal(got["tree_idxs"], want["tree_idxs"])
    for k in ("states", "next_states", "actions", "returns", "nonterminals"):
        assert np.array_equal(got[k], want[k]), k
    np.testing.assert_allclose(got["weights"], want["weights"], rtol=F32_ULP_RTOL)
    ring, blank = ora.window(want["data_idxs"])
    win = ad.windows(B)
    assert np.array_equal(win, np.where(blank, -1, ring))
    for b in range(B):
        r, bl, a, R, nt = ora.stream_window(want["data_idxs"][b])
        assert np.array_equal(np.where(bl, -1, r), win[b])
        assert a == got["actions"][b] and np.float32(R) == got["returns"][b] and np.float32(nt) == got["nonterminals"][b, 0]
    return got, want


def check_sampling(lib, mem, S, n, seed, batches=(32, 256)):
    ad, ora, rs = make_sampling_replay(lib, mem, S, n, seed)
    for B in batches:
        check_batch(ad, ora, B, rs.random_sample((64, B)), 0.5)
    ad.close()


def check_reject_near_head(lib, mem, S=16, Cs=40, B=4):
    """A draw the per-stream validity rule must reject near the write head — one whose samples the single-stream rule on the
    raw ring distance (memory.py:131 with S = 1) would have ACCEPTED — followed by the valid redraw, exact on the device."""
    ad = StreamsAdapter(lib, mem, S * Cs, 4, 3, S)
    ora = StreamsOracle(S * Cs, S, per_stream=True)
    rs = np.random.RandomState(3)
    fill(ad, ora, Cs + 9, rs, p_term=0.05, updates=False)
    tr = ora.transitions
    found = None
    for seed in range(200):
        uu = np.random.RandomState(seed).random_sample((64, B))
        trace = []
        try:
            ora.draw_indices(B, uu, trace)
        except RuntimeError:
            continue
        for idxs, probs, ok in trace[:-1]:
            naive = np.all(((tr.index - idxs) % tr.capacity > ora.n) & ((idxs - tr.index) % tr.capacity >= ora.history))
            if not ok and naive:
                found = uu
                break
        if found is not None:
            break
    assert found is not None
    got, want = check_batch(ad, ora, B, found, 0.4)
    assert want["attempts"] >= 2
    ad.close()


def check_states_at(lib, mem, S, seed, Cs=20):
    """rb_replay_states_at / rb_replay_state_at (the validation iterator) with the stream stride against the restatement, at
    every data index."""
    cap = S * Cs
    ad = StreamsAdapter(lib, mem, cap, 4, 3, S)
    ora = StreamsOracle(cap, S, per_stream=False)
    rs = np.random.RandomState(seed)
    fill(ad, ora, Cs + Cs // 2, rs, p_term=0.2, updates=False)
    got = ad.states_at(np.arange(cap))
    for i in range(cap):
        assert np.array_equal(got[i], ora.state_at(i)), i
    for i in (0, 1, S - 1, S, cap // 2 + 1, cap - 1):
        assert np.array_equal(ad.state_at(i), ora.state_at(i)), i
    ad.close()


def check_create_refusals(lib):
    """Capacity not a multiple of S, (h + n) S >= C and S outside [1, 64] are refused with a message; nothing is created."""
    for cap, h, n, S, what in ((100, 4, 3, 8, b"multiple"), (8 * 7, 4, 3, 8, b"exceed"), (8 * 6, 4, 3, 8, b"exceed"),
                               (640, 4, 3, 0, b"streams"), (65 * 10, 4, 3, 65, b"streams"), (640, 4, 3, -1, b"streams")):
        handle = C.c_void_p()
        rc = lib.rb_replay_create_streams(C.byref(handle), cap, h, n, 0.99, 0.5, 1, S)
        assert rc == -1 and not handle.value, (cap, h, n, S)
        assert what in lib.rb_last_error(), lib.rb_last_error()
    handle = C.c_void_p()
    L.check(lib, lib.rb_replay_create_streams(C.byref(handle), 8 * 8, 4, 3, 0.99, 0.5, 1, 8))
    # a whole-round replay refuses the one-transition append
    st = np.zeros((4, 84, 84), dtype=np.float32)
    assert lib.rb_replay_append(handle, st.ctypes.data, 0, 0, 0.0, 1, None) == -1
    assert b"rb_replay_append_streams" in lib.rb_last_error()
    lib.rb_replay_destroy(handle)
