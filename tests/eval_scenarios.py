"""Checks of the vectorised evaluation pieces (rb_learner_act_batch_eps, rb_tally_*) shared by the host-interpreter tests
(test_eval_emu.py) and the device tests (test_eval_gpu.py): the same code drives either build through the C ABI;
tests/eval_oracle.py is the oracle of the draw and of the tally, rb_learner_act_batch the oracle of the greedy action."""
import ctypes as C

import numpy as np

import eval_oracle as EO
from rainbow_amd import _lib as L

EPS_ROUNDS = 16          # values of rng_round of the epsilon = 0.25 check
ROW0S = (0, 5)


def pick_seed(n, epsilon=0.25, rounds=EPS_ROUNDS, A=3):
    """The first seed whose ORACLE draws (rows row0 .. row0 + n - 1, `rounds` rounds) explore a share in [0.2, 0.3] for either
    row0: a degenerate draw (nothing or everything explored) could hide a broken compare.  Decided on the CPU."""
    for seed in range(1, 200):
        shares = [np.mean([EO.eps_rows(seed, r, row0, n, epsilon, A)[0] for r in range(rounds)]) for row0 in ROW0S]
        if all(0.2 <= s <= 0.3 for s in shares):
            return seed
    raise AssertionError("no seed below 200 gives an explored share in [0.2, 0.3] at n = %d" % n)


def eval_learner(lib, mem):
    """The `k10` learner (data-efficient stack, 3 actions, history 4: the smallest the emulator tests use) with its noisy-linear
    means scaled by 8: with the plain initialisation the advantage biases decide every greedy action and all states get the
    same one."""
    from cabi_adapter import CAbiLearnAdapter
    from oracle import learner_oracle as O
    import scenarios
    cfg = O.Config(**scenarios.LEARN_CONFIGS["k10"])
    params = {k: (v * 8.0 if k.startswith("fc_") and k.endswith("weight_mu") else v) for k, v in O.init_params(cfg, 31).items()}
    ad = CAbiLearnAdapter(lib, mem, "k10")
    ad.load(params, params)
    ad.reset_noise_online(np.random.RandomState(6).randn(O.noise_draw_count(cfg)).astype(np.float32))
    return ad


def varied_states(n, history, seed=17):
    """n frame stacks that differ in structure (density, brightness, a bright block somewhere), not only in noise."""
    rs = np.random.RandomState(seed)
    st = np.zeros((n, history, 84, 84), dtype=np.float32)
    for i in range(n):
        st[i] = rs.random_sample((history, 84, 84)) * (rs.random_sample((history, 84, 84)) < rs.uniform(0.02, 1.0)) * rs.uniform(0.2, 1)
        y, x = rs.randint(0, 60, 2)
        st[i, :, y:y + 24, x:x + 24] = 1.0
    return st


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


class EpsContext:
    """One learner, one set of states on the device, and the greedy (action, q) of rb_learner_act_batch per n, computed once."""

    def __init__(self, lib, mem, n_max):
        self.lib, self.mem = lib, mem
        self.ad = eval_learner(lib, mem)
        self.A = self.ad.c["actions"]
        self.states = mem.upload(varied_states(n_max, self.ad.c["history"]))
        self._greedy = {}

    def close(self):
        self.ad.close()

    def greedy(self, n, noisy=1):
        if n not in self._greedy:
            m = self.mem
            a, q = m.empty((n,), np.int32), m.empty((n,), np.float32)
            L.check(self.lib, self.lib.rb_learner_act_batch(self.ad.h, m.ptr(self.states), n, noisy, m.ptr(a), m.ptr(q), m.stream))
            m.sync()
            self._greedy[n] = (m.download(a).astype(np.int64), m.download(q).copy())
        return self._greedy[n]

    def eps(self, n, epsilon, seed, rnd, row0, noisy=1, with_q=True, with_explored=True):
        m = self.mem
        a, q, e = m.empty((n,), np.int32), m.empty((n,), np.float32), m.empty((n,), np.uint8)
        L.check(self.lib, self.lib.rb_learner_act_batch_eps(self.ad.h, m.ptr(self.states), n, noisy, epsilon, seed, rnd, row0, m.ptr(a),
                                                            m.ptr(q) if with_q else None, m.ptr(e) if with_explored else None,
                                                            m.stream))
        m.sync()
        return m.download(a).astype(np.int64), m.download(q).copy(), m.download(e).copy()


def check_eps_zero_and_one(ctx, n, row0):
    """epsilon = 0: actions and q bit-identical to rb_learner_act_batch, nothing explored.  epsilon = 1 (and above): every
    action is the oracle's x1 % A, everything explored, q still the greedy q."""
    ga, gq = ctx.greedy(n)
    a, q, e = ctx.eps(n, 0.0, 77, 3, row0)
    assert np.array_equal(a, ga) and np.array_equal(bits(q), bits(gq)) and not e.any()
    want_e, want_a = EO.eps_rows(77, 3, row0, n, 1.0, ctx.A)
    assert want_e.all() and want_a.min() >= 0 and want_a.max() < ctx.A
    a, q, e = ctx.eps(n, 1.0, 77, 3, row0)
    assert np.array_equal(a, want_a) and e.tolist() == [1] * n and np.array_equal(bits(q), bits(gq))
    if n == 1:
        a, q, e = ctx.eps(n, 2.5, 77, 3, row0)
        assert np.array_equal(a, want_a) and e.tolist() == [1] and np.array_equal(bits(q), bits(gq))


def check_eps_quarter(ctx, n, row0, seed, rounds):
    """epsilon = 0.25: `explored` equals the oracle's decision row for row, explored rows carry the oracle's action, all other
    rows the greedy one; q is the greedy q.  (`seed` comes from pick_seed: the oracle explores 20-30 % of these draws.)"""
    ga, gq = ctx.greedy(n)
    assert len(set(ga.tolist())) >= 2, "the greedy actions of the test states are all one value: a stuck head would pass"
    for rnd in rounds:
        a, q, e = ctx.eps(n, 0.25, seed, rnd, row0)
        want_e, want_a = EO.eps_rows(seed, rnd, row0, n, 0.25, ctx.A)
        assert np.array_equal(e, want_e), (row0, rnd)
        assert np.array_equal(a, np.where(want_e == 1, want_a, ga)), (row0, rnd)
        assert np.array_equal(bits(q), bits(gq)), (row0, rnd)


def check_eps_replay(ctx, n):
    """Counter-based: the same (seed, round) again gives the same result, another round other draws; 64-bit seeds and rounds
    reach the generator whole; q_dev and explored_dev are optional."""
    A = ctx.A
    ga, _ = ctx.greedy(n)
    other_round = next(r for r in range(5, 40) if not np.array_equal(EO.eps_rows(9, 4, 0, n, 1.0, A)[1], EO.eps_rows(9, r, 0, n, 1.0, A)[1]))
    first, again, other = ctx.eps(n, 1.0, 9, 4, 0), ctx.eps(n, 1.0, 9, 4, 0), ctx.eps(n, 1.0, 9, other_round, 0)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    assert np.array_equal(first[0], EO.eps_rows(9, 4, 0, n, 1.0, A)[1])
    assert not np.array_equal(first[0], other[0]) and np.array_equal(other[0], EO.eps_rows(9, other_round, 0, n, 1.0, A)[1])
    big_seed, big_round = (1 << 63) + 12345, (1 << 40) + 7
    a, _, e = ctx.eps(n, 0.5, big_seed, big_round, 5)
    want_e, want_a = EO.eps_rows(big_seed, big_round, 5, n, 0.5, A)
    assert np.array_equal(e, want_e) and np.array_equal(a, np.where(want_e == 1, want_a, ga))
    assert want_e.tolist() != EO.eps_rows(12345, 7, 5, n, 0.5, A)[0].tolist() or want_a.tolist() != EO.eps_rows(12345, 7, 5, n, 0.5, A)[1].tolist()
    for k in (1, n):
        a, _, _ = ctx.eps(k, 1.0, 9, 4, 0, with_q=False, with_explored=False)
        assert np.array_equal(a, first[0][:k])


def check_eps_refusals(lib, mem):
    ad = eval_learner(lib, mem)
    m = mem
    st = m.upload(np.zeros((2, ad.c["history"], 84, 84), dtype=np.float32))
    a, q, e = m.upload(np.full(2, -5, dtype=np.int32)), m.empty((2,), np.float32), m.empty((2,), np.uint8)
    fn = lib.rb_learner_act_batch_eps

    def refused(word, *args):
        assert fn(*args) == -1
        msg = lib.rb_last_error()
        assert b"rb_learner_act_batch_eps" in msg and word in msg, msg

    for n in (1, 2):
        refused(b"epsilon", ad.h, m.ptr(st), n, 0, float("nan"), 1, 0, 0, m.ptr(a), m.ptr(q), m.ptr(e), m.stream)
        refused(b"epsilon", ad.h, m.ptr(st), n, 0, -0.25, 1, 0, 0, m.ptr(a), m.ptr(q), m.ptr(e), m.stream)
        refused(b"actions_dev", ad.h, m.ptr(st), n, 0, 0.5, 1, 0, 0, None, m.ptr(q), m.ptr(e), m.stream)
        refused(b"row0", ad.h, m.ptr(st), n, 0, 0.5, 1, 0, -1, m.ptr(a), m.ptr(q), m.ptr(e), m.stream)
    refused(b"NULL", None, m.ptr(st), 2, 0, 0.5, 1, 0, 0, m.ptr(a), m.ptr(q), m.ptr(e), m.stream)
    refused(b"NULL", ad.h, None, 2, 0, 0.5, 1, 0, 0, m.ptr(a), m.ptr(q), m.ptr(e), m.stream)
    refused(b"n must be", ad.h, m.ptr(st), 0, 0, 0.5, 1, 0, 0, m.ptr(a), m.ptr(q), m.ptr(e), m.stream)
    m.sync()
    assert m.download(a).tolist() == [-5, -5]                    # nothing ran
    ad.close()


# =============================================================================== tally
class TallyHandle:
    def __init__(self, lib, mem, S, E):
        self.lib, self.mem, self.S, self.E = lib, mem, S, E
        self.h = C.c_void_p()
        L.check(lib, lib.rb_tally_create(C.byref(self.h), S, E))

    def close(self):
        if self.h:
            self.lib.rb_tally_destroy(self.h)
            self.h = None

    def step(self, rewards, nonterminals):
        m = self.mem
        self._ops = (m.upload(np.asarray(rewards, dtype=np.float32)), m.upload(np.asarray(nonterminals, dtype=np.uint8)))
        L.check(self.lib, self.lib.rb_tally_step(self.h, m.ptr(self._ops[0]), m.ptr(self._ops[1]), m.stream))

    def reset(self):
        L.check(self.lib, self.lib.rb_tally_reset(self.h, self.mem.stream))

    def remaining(self):
        n = C.c_int32(-1)
        L.check(self.lib, self.lib.rb_tally_remaining(self.h, C.byref(n), self.mem.stream))
        return int(n.value)

    def result(self):
        out = np.empty(self.E, dtype=np.float32), np.full(self.E, -1, dtype=np.int32), np.full(self.E, -1, dtype=np.int32)
        L.check(self.lib, self.lib.rb_tally_read(self.h, *[x.ctypes.data for x in out], self.mem.stream))
        return out


def scripted_round(rs, S, t):
    """Step t (1-based) of the script: stream s ends an episode every 2 + 3 (s % 5) steps; rewards are never zero, so every
    ending step carries one."""
    period = 2 + 3 * (np.arange(S) % 5)
    rewards = rs.randn(S).astype(np.float32)
    rewards[rewards == 0] = 1.0
    return rewards, (t % period != 0).astype(np.uint8)


def same_record(got, want):
    (gr, gl, gs), (wr, wl, ws) = got, want
    return (np.array_equal(gr.view(np.uint32)[~np.isnan(wr)], wr.view(np.uint32)[~np.isnan(wr)])
            and np.array_equal(np.isnan(gr), np.isnan(wr)) and np.array_equal(gl, wl) and np.array_equal(gs, ws))


def check_tally_against_oracle(lib, mem, S, E, seed):
    """The scripted rounds through rb_tally_step: remaining and the whole record equal the oracle's after EVERY step (NaN in
    the unfilled slots), stepping on after remaining == 0 changes nothing, and a reset starts over."""
    rs = np.random.RandomState(seed)
    tally, ora = TallyHandle(lib, mem, S, E), EO.TallyOracle(S, E)
    assert ora.q.sum() == E and ora.q.max() - ora.q.min() <= 1
    assert tally.remaining() == E and same_record(tally.result(), ora.result())
    assert np.isnan(tally.result()[0]).all()
    for lap in range(2):
        t = 0
        while ora.remaining() > 0:
            t += 1
            rewards, nonterm = scripted_round(rs, S, t)
            tally.step(rewards, nonterm)
            ora.step(rewards, nonterm)
            assert tally.remaining() == ora.remaining(), (S, E, lap, t)
            assert same_record(tally.result(), ora.result()), (S, E, lap, t)
            assert t <= 14 * (E // S + 1)
        done = tally.result()
        assert not np.isnan(done[0]).any() and (done[1] > 0).all()
        if S > 1 and E >= S:
            assert len(set(done[1].tolist())) > 1                 # episodes of unequal length are on record
        for _ in range(15):                                       # every stream ends at least one more episode
            t += 1
            rewards, nonterm = scripted_round(rs, S, t)
            tally.step(rewards, nonterm)
            ora.step(rewards, nonterm)
        assert tally.remaining() == 0 and same_record(tally.result(), done) and same_record(ora.result(), done)
        tally.reset()
        ora.reset()
        assert tally.remaining() == E and np.isnan(tally.result()[0]).all() and same_record(tally.result(), ora.result())
    tally.close()


def check_tally_refusals(lib, mem):
    for S, E, word in ((0, 4, b"streams"), (65, 4, b"streams"), (-1, 4, b"streams"), (4, 0, b"episodes"), (4, 65537, b"episodes"),
                       (4, -3, b"episodes")):
        h = C.c_void_p()
        assert lib.rb_tally_create(C.byref(h), S, E) == -1 and not h.value
        assert b"rb_tally_create" in lib.rb_last_error() and word in lib.rb_last_error()
    assert lib.rb_tally_create(None, 4, 4) == -1 and b"rb_tally_create" in lib.rb_last_error()
    t = TallyHandle(lib, mem, 4, 6)
    rw, nt = mem.upload(np.ones(4, dtype=np.float32)), mem.upload(np.zeros(4, dtype=np.uint8))
    out = [np.zeros(6, dtype=np.float32), np.zeros(6, dtype=np.int32), np.zeros(6, dtype=np.int32)]
    n = C.c_int32(0)
    for args in ((None, mem.ptr(rw), mem.ptr(nt)), (t.h, None, mem.ptr(nt)), (t.h, mem.ptr(rw), None)):
        assert lib.rb_tally_step(*args, mem.stream) == -1
        assert b"rb_tally_step" in lib.rb_last_error() and b"NULL" in lib.rb_last_error()
    assert lib.rb_tally_reset(None, mem.stream) == -1 and b"rb_tally_reset" in lib.rb_last_error()
    assert lib.rb_tally_remaining(None, C.byref(n), mem.stream) == -1 and b"rb_tally_remaining" in lib.rb_last_error()
    assert lib.rb_tally_remaining(t.h, None, mem.stream) == -1 and b"rb_tally_remaining" in lib.rb_last_error()
    ptrs = [x.ctypes.data for x in out]
    for missing in range(3):
        args = list(ptrs)
        args[missing] = None
        assert lib.rb_tally_read(t.h, *args, mem.stream) == -1 and b"rb_tally_read" in lib.rb_last_error()
    assert lib.rb_tally_read(None, *ptrs, mem.stream) == -1
    assert t.remaining() == 6                                     # nothing ran
    # the largest tally: 65536 slots over 64 streams
    big = TallyHandle(lib, mem, 64, 65536)
    big.step(np.full(64, 2.0, dtype=np.float32), np.zeros(64, dtype=np.uint8))
    assert big.remaining() == 65536 - 64
    r, ln, st = big.result()
    assert np.array_equal(np.flatnonzero(~np.isnan(r)), np.arange(64) * 1024) and ln.sum() == 64 and st[-1] == 63 and st[1024] == 1
    big.close()
    assert lib.rb_tally_destroy(None) == 0
    t.close()
