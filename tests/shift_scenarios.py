"""Checks of the random-shift frame-stack gather (rb_replay_gather_shifted) shared by the host-interpreter tests
(test_shift_emu.py) and the device tests (test_shift_gpu.py): the same code drives either build through the C ABI,
tests/shift_oracle.py is the oracle.  Every comparison of stacks and shifts is exact equality (the output is uint8)."""
import numpy as np

import scenarios
import shift_oracle as SO
from cabi_adapter import CAbiLearnAdapter, CAbiReplayAdapter
from rainbow_amd import _lib as L
from streams_scenarios import StreamsAdapter

ATTEMPTS = 8


def frame_of(ordinal):
    """Frame of the ordinal-th append: every row, column and slot distinguishable (17 and 31 are units mod 251, so neighbouring
    rows / columns / frames never agree along a line): a wrong row, column or an off-by-one at a dword seam shows."""
    y, x = np.mgrid[0:84, 0:84]
    return ((17 * y + 31 * x + 7 * int(ordinal)) % 251).astype(np.uint8)


class ShiftReplay:
    """A small replay filled past one wrap with episode ends every few transitions of each stream, the slots a draw may not
    use given zero priority (so that nine strata of a 64-slot ring all hold valid leaves), and a host copy of the ring."""

    def __init__(self, lib, mem, capacity, history, n, streams=1, seed=7, appends=None, rs_seed=1):
        self.lib, self.mem = lib, mem
        self.C, self.h, self.n, self.S, self.seed = capacity, history, n, streams, seed
        if streams == 1:
            self.ad = CAbiReplayAdapter(lib, mem, capacity, history, n, 0.99, 0.5, seed=seed)
        else:
            self.ad = StreamsAdapter(lib, mem, capacity, history, n, streams, seed=seed)
        rs = np.random.RandomState(rs_seed)
        total = appends if appends is not None else capacity + (capacity // 3) // streams * streams
        assert total % streams == 0 and total > capacity
        ts, nt = np.zeros(total, np.int32), np.ones(total, np.uint8)
        t, left = np.zeros(streams, np.int64), rs.randint(2, 9, size=streams)        # per stream: episode step, steps left
        for k in range(total):
            s = k % streams
            ts[k] = t[s]
            left[s] -= 1
            if left[s] == 0:
                nt[k], t[s], left[s] = 0, 0, rs.randint(2, 9)
            else:
                t[s] += 1
        frames = np.stack([frame_of(k) for k in range(total)])
        actions, rewards = rs.randint(0, 3, total).astype(np.int32), rs.choice([-1.0, 0.0, 1.0], size=total).astype(np.float32)
        step = capacity // 2 // streams * streams                                     # (an append takes at most `capacity` rows)
        for lo in range(0, total, step):
            sl = slice(lo, min(total, lo + step))
            self.ad.append_batch(frames[sl], ts[sl], actions[sl], rewards[sl], nt[sl])
        self.ring = np.zeros((capacity, 84, 84), np.uint8)
        for k in range(total):
            self.ring[k % capacity] = frames[k]
        index = total % capacity
        idx = np.arange(capacity)
        d, e = (index - idx) % capacity, (idx - index) % capacity
        valid = (d > n * streams) & (d <= capacity - streams) & (e >= history * streams)     # replay_sample.h, memory.py:131
        assert valid.sum() >= 16
        bad = idx[~valid] + self.ad.bufs.tree_start
        self.ad.update_leaves(bad, np.zeros(len(bad), np.float32))

    def close(self):
        self.ad.close()

    def draw(self, batch, uu, with_stacks=False):
        """rb_replay_sample with injected uniforms; NULL stacks unless with_stacks.  Returns the device buffers of the scalars (and
        the plain stacks)."""
        m, h = self.mem, self.h
        o = dict(tree_idx=m.empty((batch,), np.int64), actions=m.empty((batch,), np.int64), returns=m.empty((batch,), np.float32),
                 nonterm=m.empty((batch,), np.float32), weights=m.empty((batch,), np.float32), uu=m.upload(np.asarray(uu, np.float64)))
        st = ns = None
        if with_stacks:
            st, ns = m.empty((batch, h, 84, 84), np.uint8), m.empty((batch, h, 84, 84), np.uint8)
        L.check(self.lib, self.lib.rb_replay_sample(self.ad.h, batch, 0.5, m.ptr(o["uu"]), int(np.asarray(uu).shape[0]), m.ptr(o["tree_idx"]),
                                                    m.ptr(st), m.ptr(ns), m.ptr(o["actions"]), m.ptr(o["returns"]), m.ptr(o["nonterm"]),
                                                    m.ptr(o["weights"]), m.stream))
        m.sync()
        hdr = self.ad.raw_header()
        assert hdr.last_status == 0, "the draw gave up after %d attempts" % hdr.last_attempts
        o["states"], o["next_states"] = st, ns
        return o

    def reference_stacks(self, batch):
        """The un-shifted stacks of the last draw from its window table and the host copy of the ring (memory.py:136-138)."""
        win = self.mem.view(self.ad.bufs.window_dev, (batch, self.h + self.n), np.int32)
        assert win.max() < self.C

        def stack(cols):
            w = win[:, cols]
            return np.where((w < 0)[:, :, None, None], np.uint8(0), self.ring[np.maximum(w, 0)])

        return stack(slice(0, self.h)), stack(slice(self.n, self.n + self.h)), win

    def gather(self, batch, pad, draw=0, shifts=None, want_shifts=True):
        """rb_replay_gather_shifted on the last draw -> (states, next_states, shifts_out) on the host."""
        m, h = self.mem, self.h
        st, ns = m.empty((batch, h, 84, 84), np.uint8), m.empty((batch, h, 84, 84), np.uint8)
        sin = m.upload(np.ascontiguousarray(shifts, dtype=np.int8).view(np.uint8)) if shifts is not None else None
        sout = m.upload(np.full((batch, 2, 2), 0x55, np.uint8)) if want_shifts else None
        L.check(self.lib, self.lib.rb_replay_gather_shifted(self.ad.h, batch, pad, draw, m.ptr(sin), m.ptr(st), m.ptr(ns), m.ptr(sout),
                                                            m.stream))
        m.sync()
        self.last_dev = (st, ns)
        return m.download(st), m.download(ns), (m.download(sout).view(np.int8) if want_shifts else None)


def all_pairs(pad):
    r = np.arange(-pad, pad + 1)
    return np.array([(dy, dx) for dy in r for dx in r], dtype=np.int8)


# =============================================================================== 1. kernel against the oracle, injected shifts
def check_injected_enumeration(lib, mem, history, n, pad, streams=1, batch=9):
    """The full enumeration of (dy, dx) in [-pad, pad]^2 spread over successive calls of 2 x batch stacks each, a fresh draw per call,
    on a 64-slot replay (66 with 3 streams) with blanked slots in both stacks."""
    cap = 64 if streams == 1 else 66
    rp = ShiftReplay(lib, mem, cap, history, n, streams=streams, rs_seed=10 * history + n)
    pairs = all_pairs(pad)
    per_call = 2 * batch
    calls = max(4, -(-len(pairs) // per_call))        # (pad 1 is 9 pairs: a few more draws, so that blanked slots do occur)
    rs = np.random.RandomState(pad)
    blank_state = blank_next = 0
    for k in range(calls):
        shifts = pairs[(k * per_call + np.arange(per_call)) % len(pairs)].reshape(batch, 2, 2)
        rp.draw(batch, rs.random_sample((ATTEMPTS, batch)))
        ref_s, ref_n, win = rp.reference_stacks(batch)
        blank_state += int((win[:, :history] < 0).sum())
        blank_next += int((win[:, n:n + history] < 0).sum())
        got_s, got_n, got_shifts = rp.gather(batch, pad, shifts=shifts)
        want_s, want_n = SO.shift_batch(ref_s, ref_n, shifts)
        assert np.array_equal(got_shifts, shifts), k
        assert np.array_equal(got_s, want_s), (k, shifts[:, 0].tolist())
        assert np.array_equal(got_n, want_n), (k, shifts[:, 1].tolist())
    if history > 1:
        assert blank_state > 0 and blank_next > 0, "the scenario must blank slots in both stacks"
    else:
        assert blank_next > 0
    rp.close()


# =============================================================================== 2. pad = 0
def check_pad_zero_is_the_plain_gather(lib, mem, history=4, n=3, batch=9):
    """The shifted gather with pad = 0 (device shifts and injected non-zero shifts, which pad = 0 clamps away) writes the bytes
    rb_replay_sample writes when handed stack pointers — same injected uniforms, twin replays."""
    a, b = ShiftReplay(lib, mem, 64, history, n), ShiftReplay(lib, mem, 64, history, n)
    uu = np.random.RandomState(2).random_sample((ATTEMPTS, batch))
    plain = a.draw(batch, uu, with_stacks=True)
    b.draw(batch, uu)
    ps, pn = mem.download(plain["states"]), mem.download(plain["next_states"])
    ref_s, ref_n, _ = b.reference_stacks(batch)
    assert np.array_equal(ps, ref_s) and np.array_equal(pn, ref_n)
    got_s, got_n, sh = b.gather(batch, 0, draw=3)
    assert np.array_equal(got_s, ps) and np.array_equal(got_n, pn) and not sh.any()
    got_s, got_n, sh = b.gather(batch, 0, shifts=np.full((batch, 2, 2), 3, np.int8))
    assert np.array_equal(got_s, ps) and np.array_equal(got_n, pn) and not sh.any()
    got_s, got_n, _ = a.gather(batch, 0, want_shifts=False)       # (after a draw that was handed stack pointers: the same table)
    assert np.array_equal(got_s, ps) and np.array_equal(got_n, pn)
    a.close(); b.close()


# =============================================================================== 3. Philox path
def check_philox_path(lib, mem, seed, pad=4, batch=32):
    """shifts_in = NULL: shifts_out is the oracle's draw for (seed, draw, i), the stacks are the oracle's under those shifts, the same
    (seed, draw) gives the same bytes twice, and the replay header (rng_counter included) is bit-identical around the call."""
    rp = ShiftReplay(lib, mem, 256, 4, 3, seed=seed, appends=300)
    rp.draw(batch, np.random.RandomState(3).random_sample((ATTEMPTS, batch)))
    ref_s, ref_n, _ = rp.reference_stacks(batch)
    seen = []
    for draw in (0, 1, 2 ** 32 + 5):
        hdr0 = bytes(rp.ad.raw_header())
        got_s, got_n, got_shifts = rp.gather(batch, pad, draw=draw)
        assert bytes(rp.ad.raw_header()) == hdr0, "the header changed"
        want_shifts = SO.draw_shifts(seed, draw, batch, pad)
        assert np.array_equal(got_shifts, want_shifts), draw
        want_s, want_n = SO.shift_batch(ref_s, ref_n, want_shifts)
        assert np.array_equal(got_s, want_s) and np.array_equal(got_n, want_n), draw
        again_s, again_n, again_shifts = rp.gather(batch, pad, draw=draw)
        assert np.array_equal(again_s, got_s) and np.array_equal(again_n, got_n) and np.array_equal(again_shifts, got_shifts)
        seen.append(got_shifts)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2])
    assert np.abs(np.stack(seen)).max() == pad and len(np.unique(np.stack(seen))) == 2 * pad + 1      # the whole range is reached
    rp.close()
    return seen


# =============================================================================== 4. guard bands
def check_guard_bands(lib, guarded_mem, pad=8, batch=5):
    """pad = 8 on canaried caller buffers (tests/guarded_mem.py): the extreme shifts injected, then the device draw; no band
    around the stacks or the shift buffers is written."""
    rp = ShiftReplay(lib, guarded_mem, 64, 4, 3)
    rp.draw(batch, np.random.RandomState(4).random_sample((ATTEMPTS, batch)))
    ref_s, ref_n, _ = rp.reference_stacks(batch)
    corners = np.array([[[-8, -8], [8, 8]], [[-8, 8], [8, -8]], [[0, 8], [8, 0]], [[-8, 0], [0, -8]], [[7, -5], [-3, 6]]], np.int8)
    got_s, got_n, sh = rp.gather(batch, pad, shifts=corners)
    want_s, want_n = SO.shift_batch(ref_s, ref_n, corners)
    assert np.array_equal(sh, corners) and np.array_equal(got_s, want_s) and np.array_equal(got_n, want_n)
    rp.gather(batch, pad, draw=9)
    n, bad = guarded_mem.check()
    assert n >= 8 and len(bad) == 0, bad
    rp.close()


# =============================================================================== 5. refusals
def check_refusals(lib, mem, batch=4):
    """pad = -1, pad = 9, a NULL stack, batch = 0 (and a NULL handle): a negative return code, a message that names the argument,
    and nothing launched (the output buffers keep their fill)."""
    rp = ShiftReplay(lib, mem, 64, 4, 3)
    rp.draw(batch, np.random.RandomState(5).random_sample((ATTEMPTS, batch)))
    st, ns = mem.upload(np.full((batch, 4, 84, 84), 0xAB, np.uint8)), mem.upload(np.full((batch, 4, 84, 84), 0xAB, np.uint8))
    so = mem.upload(np.full((batch, 2, 2), 0x55, np.uint8))
    p = mem.ptr
    cases = [((rp.ad.h, batch, -1, 0, None, p(st), p(ns), p(so)), "pad"), ((rp.ad.h, batch, 9, 0, None, p(st), p(ns), p(so)), "pad"),
             ((rp.ad.h, batch, 4, 0, None, None, p(ns), p(so)), "states_dev"), ((rp.ad.h, batch, 4, 0, None, p(st), None, p(so)), "next_states_dev"),
             ((rp.ad.h, 0, 4, 0, None, p(st), p(ns), p(so)), "batch"), ((rp.ad.h, 1025, 4, 0, None, p(st), p(ns), p(so)), "batch"),
             ((None, batch, 4, 0, None, p(st), p(ns), p(so)), "handle")]
    for args, word in cases:
        rc = lib.rb_replay_gather_shifted(*args, mem.stream)
        assert rc < 0, (word, rc)
        assert word in lib.rb_last_error().decode() and "rb_replay_gather_shifted" in lib.rb_last_error().decode(), (word, lib.rb_last_error())
    mem.sync()
    assert (mem.download(st) == 0xAB).all() and (mem.download(ns) == 0xAB).all() and (mem.download(so) == 0x55).all()
    L.check(lib, lib.rb_replay_gather_shifted(rp.ad.h, batch, 8, 0, None, p(st), p(ns), None, mem.stream))     # the limits themselves pass
    rp.close()


# =============================================================================== 7. the learn step
def check_learn_step(lib, mem, name="k10", pad=4, seed=7):
    """sample (NULL stacks) -> shifted gather (pad 4, draw 0, device shifts) -> rb_learner_learn on the gathered device buffers, then
    clip + Adam, against the oracle's learn step on the oracle-shifted stacks: the trace comparison of helpers.py, unchanged."""
    from adapters import OracleLearnAdapter
    from helpers import assert_learn_trace_matches
    from oracle import learner_oracle as O
    c = scenarios.LEARN_CONFIGS[name]
    B, h, n = c["batch"], c["history"], c["multi_step"]
    cfg = O.Config(**c)
    rp = ShiftReplay(lib, mem, 64, h, n, seed=seed)
    o = rp.draw(B, np.random.RandomState(6).random_sample((ATTEMPTS, B)))
    ref_s, ref_n, _ = rp.reference_stacks(B)
    got_s, got_n, got_shifts = rp.gather(B, pad, draw=0)
    st_dev, ns_dev = rp.last_dev
    shifts = SO.draw_shifts(seed, 0, B, pad)
    want_s, want_n = SO.shift_batch(ref_s, ref_n, shifts)
    assert np.array_equal(got_shifts, shifts) and shifts.any()
    assert np.array_equal(got_s, want_s) and np.array_equal(got_n, want_n)
    assert not np.array_equal(want_s, ref_s)
    online, target = O.init_params(cfg, 41), O.init_params(cfg, 42)
    draws = O.noise_draw_count(cfg)
    rs = np.random.RandomState(8)
    raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
    ad = CAbiLearnAdapter(lib, mem, name)
    ora = OracleLearnAdapter(name)
    for be in (ad, ora):
        be.load(online, target)
        be.reset_noise_online(raw_on)
    r = mem.upload(raw_tg)
    L.check(lib, lib.rb_learner_reset_noise(ad.h, 1, mem.ptr(r), mem.stream))
    ad._loss = mem.empty((B,), np.float32)
    L.check(lib, lib.rb_learner_learn(ad.h, mem.ptr(st_dev), mem.ptr(ns_dev), mem.ptr(o["actions"]), mem.ptr(o["returns"]),
                                      mem.ptr(o["nonterm"]), mem.ptr(o["weights"]), mem.ptr(ad._loss), mem.stream))
    got = ad.finish_step()
    batch = dict(states=want_s, next_states=want_n, actions=mem.download(o["actions"]), returns=mem.download(o["returns"]),
                 nonterminals=mem.download(o["nonterm"]), weights=mem.download(o["weights"]))
    want = ora.learn_step(batch, raw_tg)

    def trace(out, params):
        t = {"s0_loss": np.asarray(out["loss"], np.float32), "s0_grad_norm": np.float32(out["grad_norm"])}
        for k, g in out["grads"].items():
            t["s0_grad/" + k] = scenarios.summarize(g)
        for k, p in params.items():
            t["s0_param/" + k] = scenarios.summarize(p)
        return t

    assert_learn_trace_matches(trace(got, ad.params()), trace(want, ora.params()), label="shifted-learn/" + name)
    # (the un-shifted stacks give another loss: the comparison above does tell the two apart)
    plain = OracleLearnAdapter(name)
    plain.load(online, target)
    plain.reset_noise_online(raw_on)
    other = plain.learn_step(dict(batch, states=ref_s, next_states=ref_n), raw_tg)
    assert not np.allclose(other["loss"], want["loss"], rtol=2e-5, atol=1e-7)
    ad.close(); rp.close()
