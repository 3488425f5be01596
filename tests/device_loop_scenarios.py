"""Checks of the device-resident actor loop (rb_replay_append_streams_dev, rb_catch_*) shared by the host-interpreter tests
(test_device_loop_emu.py) and the device tests (test_device_loop_gpu.py): the same code drives either build through the C
ABI; tests/catch_oracle.py is the environment's oracle, the host-operand round (rb_replay_append_streams) the replay's."""
import ctypes as C

import numpy as np

import catch_oracle as CO
from rainbow_amd import _lib as L
from streams_scenarios import StreamsAdapter

HEADER_FIELDS = [f for f, _ in L.ReplayHeader._fields_]


class DevRoundAdapter(StreamsAdapter):
    """StreamsAdapter + the device-operand round: the per-stream episode timesteps live in a device vector the kernel updates."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.ts_dev = self.mem.upload(np.zeros(self.streams, dtype=np.int32))

    def append_round_dev(self, states, actions, rewards, terminals):
        m = self.mem
        st = m.upload(np.asarray(states, dtype=np.float32))
        ops = [m.upload(np.asarray(actions, dtype=np.int32)), m.upload(np.asarray(rewards, dtype=np.float32)),
               m.upload((~np.asarray(terminals, dtype=bool)).astype(np.uint8))]
        L.check(self.lib, self.lib.rb_replay_append_streams_dev(self.h, m.ptr(st), m.ptr(self.ts_dev), *[m.ptr(o) for o in ops],
                                                                m.stream))
        m.sync()

    def timesteps_dev(self):
        return self.mem.download(self.ts_dev).copy()

    def push_timesteps(self):
        """host rounds were appended: the device vector continues from the host's counters"""
        self.ts_dev = self.mem.upload(self.stream_t.astype(np.int32))

    def pull_timesteps(self):
        self.stream_t = self.timesteps_dev()


def header_values(ad):
    hdr = ad.raw_header()
    return [getattr(hdr, f) for f in HEADER_FIELDS]      # (field by field: the struct's padding bytes are never written)


def assert_identical(a, b, label):
    ca, cb = a.columns(), b.columns()
    for k in ca:
        assert np.array_equal(ca[k], cb[k]), (label, k)
    assert np.array_equal(a.tree(), b.tree()), label
    assert header_values(a) == header_values(b), label
    pa, pb = [], []
    for ad, out in ((a, pa), (b, pb)):
        idx, full = C.c_int64(-1), C.c_int32(-1)
        L.check(ad.lib, ad.lib.rb_replay_position(ad.h, C.byref(idx), C.byref(full)))
        out += [idx.value, full.value]
    assert pa == pb, label


def check_append_dev_equals_host(lib, mem, S, seed, history=4, n=3, capacity=None, rounds=None, check_every=1):
    """The same rounds through rb_replay_append_streams (host operands), rb_replay_append_streams_dev (device operands) and a
    third replay that alternates between the two: frames, columns, the whole tree and the header bit-identical after every
    round (the ring wraps at least three times), and the in/out timestep vector follows memory.py:108 per stream."""
    Cs = 2 * (history + n) + 2
    cap = S * Cs if capacity is None else capacity
    rounds = 3 * Cs + 5 if rounds is None else rounds
    rs = np.random.RandomState(seed)
    host = DevRoundAdapter(lib, mem, cap, history, n, S)
    dev = DevRoundAdapter(lib, mem, cap, history, n, S)
    mix = DevRoundAdapter(lib, mem, cap, history, n, S)
    tree_start = int(host.bufs.tree_start)
    mix_on_device = False
    for r in range(rounds):
        states = np.zeros((S, history, 84, 84), dtype=np.float32)             # (a round stores state[s][history - 1] only)
        states[:, -1] = rs.random_sample((S, 84, 84)).astype(np.float32)
        if r % 3 == 0:
            states[:, -1] = rs.randint(0, 256, size=(S, 84, 84)).astype(np.float32) / np.float32(255)
        actions = rs.randint(0, 6, S)
        rewards = rs.choice([-1.0, 0.0, 0.5, 1.0], size=S).astype(np.float32)
        terms = rs.random_sample(S) < 0.15
        want_t = np.where(terms, 0, host.stream_t + 1).astype(np.int32)
        host.append_round(states, actions, rewards, terms)
        dev.append_round_dev(states, actions, rewards, terms)
        go_device = (r // 3) % 2 == 1                                           # three host rounds, three device rounds, ...
        if go_device and not mix_on_device:
            mix.push_timesteps()
        if not go_device and mix_on_device:
            mix.pull_timesteps()
        mix_on_device = go_device
        if go_device:
            mix.append_round_dev(states, actions, rewards, terms)
        else:
            mix.append_round(states, actions, rewards, terms)
        assert np.array_equal(host.stream_t, want_t)
        assert np.array_equal(dev.timesteps_dev(), want_t), r
        if r % 7 == 3:                                                          # the running max moves
            k = min(64, cap)
            idx = rs.randint(0, cap, k) + tree_start
            vals = (rs.random_sample(k) * 3 + 0.05).astype(np.float32)
            for ad in (host, dev, mix):
                ad.update_leaves(idx, vals)
        if r % check_every == 0 or r == rounds - 1:
            assert_identical(host, dev, "S=%d round %d host/device" % (S, r))
            assert_identical(host, mix, "S=%d round %d host/interleaved" % (S, r))
    if capacity is None:
        assert rounds * S >= 3 * cap
    if mix_on_device:
        mix.pull_timesteps()
    assert np.array_equal(mix.stream_t, host.stream_t)
    for ad in (host, dev, mix):
        ad.close()


def check_append_dev_refusals(lib, mem):
    """NULL operands, a misaligned state pointer and a write head off the round boundary: RB_ERR_INVALID, the entry point named."""
    S = 4
    ad = DevRoundAdapter(lib, mem, S * 16, 4, 3, S)
    st = mem.upload(np.zeros((S, 4, 84, 84), dtype=np.float32).reshape(-1))
    pad = mem.upload(np.zeros(S * 4 * 84 * 84 + 4, dtype=np.float32))
    ac, rw, nt = (mem.upload(np.zeros(S, dtype=d)) for d in (np.int32, np.float32, np.uint8))
    good = [mem.ptr(st), mem.ptr(ad.ts_dev), mem.ptr(ac), mem.ptr(rw), mem.ptr(nt)]
    for missing in range(5):
        args = list(good)
        args[missing] = None
        assert lib.rb_replay_append_streams_dev(ad.h, *args, mem.stream) == -1
        assert b"rb_replay_append_streams_dev" in lib.rb_last_error() and b"NULL" in lib.rb_last_error()
    assert lib.rb_replay_append_streams_dev(None, *good, mem.stream) == -1
    assert b"rb_replay_append_streams_dev" in lib.rb_last_error()
    assert lib.rb_replay_append_streams_dev(ad.h, mem.ptr(pad) + 4, *good[1:], mem.stream) == -1
    assert b"rb_replay_append_streams_dev" in lib.rb_last_error() and b"aligned" in lib.rb_last_error()
    # a write head that is not a multiple of S (a restored header): both round entry points refuse
    hdr = ad.raw_header()
    hdr.index = 1
    raw = np.frombuffer(bytes(hdr), dtype=np.uint8).copy()
    L.check(lib, lib.rb_copy_to_device(ad.bufs.header_dev, raw.ctypes.data, raw.nbytes, mem.stream))
    ad.raw_header()                                       # (resynchronises the library's host mirror of the write head)
    assert lib.rb_replay_append_streams_dev(ad.h, *good, mem.stream) == -1
    assert b"rb_replay_append_streams_dev" in lib.rb_last_error() and b"round boundary" in lib.rb_last_error()
    mem.sync()
    assert np.array_equal(mem.download(ad.ts_dev), np.zeros(S, dtype=np.int32))       # nothing ran
    ad.close()


# =============================================================================== Catch
class CatchHandle:
    """rb_catch_* through the C ABI with two stack buffers swapped by the caller."""

    def __init__(self, lib, mem, S, history, seed):
        self.lib, self.mem, self.S, self.history = lib, mem, S, history
        self.h = C.c_void_p()
        L.check(lib, lib.rb_catch_create(C.byref(self.h), S, history, seed))
        self.bufs = [mem.empty((S, history, 84, 84), np.float32) for _ in range(2)]
        self.cur = 0
        self.rewards = mem.empty((S,), np.float32)
        self.nonterminals = mem.empty((S,), np.uint8)

    def close(self):
        if self.h:
            self.lib.rb_catch_destroy(self.h)
            self.h = None

    def stacks(self):
        return self.bufs[self.cur]

    def reset(self):
        L.check(self.lib, self.lib.rb_catch_reset(self.h, self.mem.ptr(self.bufs[self.cur]), self.mem.stream))
        self.mem.sync()
        return self.mem.download(self.bufs[self.cur])

    def step_dev(self, actions_buf):
        """actions already on the device; no download"""
        m = self.mem
        L.check(self.lib, self.lib.rb_catch_step(self.h, m.ptr(actions_buf), m.ptr(self.bufs[self.cur]), m.ptr(self.bufs[self.cur ^ 1]),
                                                 m.ptr(self.rewards), m.ptr(self.nonterminals), m.stream))
        self.cur ^= 1

    def step(self, actions):
        m = self.mem
        self._ac = m.upload(np.asarray(actions, dtype=np.int32))
        self.step_dev(self._ac)
        m.sync()
        return m.download(self.bufs[self.cur]), m.download(self.rewards).copy(), m.download(self.nonterminals).copy()

    def stats(self):
        st = L.CatchStats()
        L.check(self.lib, self.lib.rb_catch_stats(self.h, C.byref(st), self.mem.stream))
        return dict(episodes=int(st.episodes), catches=int(st.catches), return_sum=float(st.return_sum))

    def reset_stats(self):
        L.check(self.lib, self.lib.rb_catch_reset_stats(self.h, self.mem.stream))


def random_actions(rs, S):
    """Mostly the three moves, now and then a value outside [0, 3) (counts as stay)."""
    a = rs.randint(0, 3, S)
    odd = rs.random_sample(S) < 0.1
    return np.where(odd, rs.choice([-1, 3, 7, 1 << 20, -(1 << 31)], size=S), a).astype(np.int64)


def check_catch_against_oracle(lib, mem, S, history, seed, rounds=60):
    """`rounds` steps of random actions (several episode ends per stream): stacks bit-identical, rewards, nonterminals and the
    accumulated totals equal; a manual reset in between starts every stream's next episode in both."""
    rs = np.random.RandomState(seed)
    env, ora = CatchHandle(lib, mem, S, history, seed), CO.CatchOracle(S, history, seed)
    assert np.array_equal(env.reset(), ora.reset())
    ends = np.zeros(S, dtype=int)
    for r in range(rounds):
        actions = random_actions(rs, S)
        got_st, got_rw, got_nt = env.step(actions)
        want_st, want_rw, want_term = ora.step(actions)
        assert np.array_equal(got_st, want_st), (S, history, r)
        assert np.array_equal(got_rw, want_rw) and np.array_equal(got_nt.astype(bool), ~want_term), (S, history, r)
        ends += want_term
        if r == 25:
            assert env.stats() == ora.stats()
            assert np.array_equal(env.reset(), ora.reset())          # mid-episode restart
        if r == 40:
            env.reset_stats(); ora.reset_stats()
    assert ends.min() >= 3
    assert env.stats() == ora.stats() and env.stats()["episodes"] > 0
    env.close()


def check_catch_seeds_and_refusals(lib, mem):
    a, b, c = CatchHandle(lib, mem, 7, 4, 11), CatchHandle(lib, mem, 7, 4, 11), CatchHandle(lib, mem, 7, 4, 12)
    sa, sb, sc = a.reset(), b.reset(), c.reset()
    assert np.array_equal(sa, sb) and not np.array_equal(sa, sc)
    rs = np.random.RandomState(0)
    differ = False
    for r in range(30):
        actions = rs.randint(0, 3, 7)
        xa, xb, xc = a.step(actions), b.step(actions), c.step(actions)
        for u, v in zip(xa, xb):
            assert np.array_equal(u, v)
        differ |= not np.array_equal(xa[0], xc[0])
    assert differ and a.stats() == b.stats()
    for bad in (0, 65, -1):
        h = C.c_void_p()
        assert lib.rb_catch_create(C.byref(h), bad, 4, 1) == -1 and not h.value
        assert b"rb_catch_create" in lib.rb_last_error() and b"streams" in lib.rb_last_error()
    h = C.c_void_p()
    assert lib.rb_catch_create(C.byref(h), 4, 0, 1) == -1 and b"history" in lib.rb_last_error()
    # a step before the first reset, and an in-place step, are refused
    d = CatchHandle(lib, mem, 2, 4, 1)
    ac = mem.upload(np.zeros(2, dtype=np.int32))
    args = [mem.ptr(ac), mem.ptr(d.bufs[0]), mem.ptr(d.bufs[1]), mem.ptr(d.rewards), mem.ptr(d.nonterminals)]
    assert lib.rb_catch_step(d.h, *args, mem.stream) == -4 and b"rb_catch_reset" in lib.rb_last_error()
    d.reset()
    args[2] = args[1]
    assert lib.rb_catch_step(d.h, *args, mem.stream) == -1 and b"overlaps" in lib.rb_last_error()
    for x in (a, b, c, d):
        x.close()


def check_random_policy_is_poor(lib, mem, S=64, rounds=11 * 40):
    """Sanity of the game itself: uniformly random actions neither win nor lose it outright (the paddle covers 3 of 12 columns
    and drifts at random: the mean return has to lie well inside (-1, 1), on the losing side), and the device's totals are the oracle's."""
    rs = np.random.RandomState(1)
    env, ora = CatchHandle(lib, mem, S, 1, 99), CO.CatchOracle(S, 1, 99)
    env.reset(); ora.reset()
    for r in range(rounds):
        actions = rs.randint(0, 3, S)
        ora.step(actions)
        ac = mem.upload(actions.astype(np.int32))
        env.step_dev(ac)                                   # (no download: the totals stay on the device)
    st = env.stats()
    assert st == ora.stats()
    assert st["episodes"] == S * 40 and -0.8 < st["return_sum"] / st["episodes"] < -0.1
    env.close()


# =============================================================================== a whole round
def check_device_round(lib, mem, make_learner, S=3, rounds=14, seed=4):
    """act_batch -> rb_catch_step -> rb_replay_append_streams_dev with nothing read back in between, against the same rounds
    through the host-operand append with the oracle environment and the same actions: replays bit-identical, the device
    timestep vector equal to the host's counters."""
    ad = make_learner()
    history, n = ad.c["history"], ad.c["multi_step"]
    cap = S * (2 * (history + n) + 2)
    env, ora = CatchHandle(lib, mem, S, history, seed), CO.CatchOracle(S, history, seed)
    dev = DevRoundAdapter(lib, mem, cap, history, n, S)
    host = DevRoundAdapter(lib, mem, cap, history, n, S)
    env.reset()
    stacks = ora.reset()
    actions_dev = mem.empty((S,), np.int32)
    ended = 0
    for r in range(rounds):
        L.check(lib, lib.rb_learner_act_batch(ad.h, mem.ptr(env.stacks()), S, 1, mem.ptr(actions_dev), None, mem.stream))
        acted_on = env.stacks()
        env.step_dev(actions_dev)
        L.check(lib, lib.rb_replay_append_streams_dev(dev.h, mem.ptr(acted_on), mem.ptr(dev.ts_dev), mem.ptr(actions_dev),
                                                      mem.ptr(env.rewards), mem.ptr(env.nonterminals), mem.stream))
        mem.sync()
        actions = mem.download(actions_dev).copy()          # (read back for the host-driven twin only)
        assert actions.min() >= 0 and actions.max() < CO.ACTIONS
        nxt, rewards, terms = ora.step(actions)
        host.append_round(stacks, actions, rewards, terms)
        stacks = nxt
        ended += int(terms.sum())
        assert np.array_equal(mem.download(env.stacks()), stacks), r
        assert_identical(host, dev, "round %d" % r)
        assert np.array_equal(dev.timesteps_dev(), host.stream_t)
    assert ended >= S
    assert env.stats() == ora.stats()
    for x in (env, dev, host, ad):
        x.close()
