"""Checks of the annealed update horizon and discount (rb_replay_set_horizon / rb_learner_set_horizon) shared by the host-interpreter
tests (test_horizon_emu.py, the small rows) and the device tests (test_horizon_gpu.py, every row): the same code drives either
build through the C ABI.

A. Replay.  The device replay is created with n_max and then set to (n_eff, gamma); the oracle is tests/streams_oracle.py's
restatement (oracle.replay_oracle's storage, tree, search and n-step arithmetic; one stream is the plain ReplayOracle rule) BUILT
with multi_step = n_eff and that gamma, fed the same appends, priorities and injected uniforms.  Every output is compared with
np.array_equal: tree indices, actions, returns, nonterminals, weights, both gathered stacks, the attempt count and the window table
with its -1 tail.  Priorities are 1 on every slot a draw may use and 0 elsewhere (appends store the running maximum, which stays 1),
so that every sampled leaf has the same probability: the importance weights are then x / x = 1 on both sides whatever the last bit
of the machine's float32 power is (helpers.F32_ULP_RTOL says why the existing parity tests allow them 4 ulp; here they are held bit
for bit), and a stratum of a 96-slot ring never lies wholly inside the write head's exclusion zone.

B. Learner.  tests/learn_steps.py's two-step run (OracleRun, the device's conv ReLU decisions handed to the oracle, the hidden ReLU
margin asserted, helpers.assert_learn_trace_matches unchanged): the learner is created with multi_step 10 and set to (3, 0.997)
before step 0 and to (7, 0.98) before step 1, the oracle's Config carries the same (n, gamma) per step.  Seeds: the first from 0 for
which the oracle alone gives both steps a hidden margin of 2.5 x RELU_MARGIN (shape_range_scenarios' rule; LEARN_ROWS has the
margins the search printed on the CPU)."""
import ctypes as C

import numpy as np

import scenarios
import shift_oracle as SO
from cabi_adapter import CAbiLearnAdapter
from head_shapes_scenarios import make_learner
from helpers import assert_learn_trace_matches
from learn_steps import RELU_MARGIN, OracleRun, conv_shapes, two_step_inputs
from oracle import learner_oracle as O
from rainbow_amd import _lib as L
from streams_oracle import StreamsOracle
from streams_scenarios import StreamsAdapter

ATTEMPTS = 8
G0 = 0.97           # the discount the replays are created with (BBF's start)
GAMMA = 0.997       # the discount set_horizon installs unless the row says otherwise

# A1: (history, n_max, n_eff, streams, capacity, batch).  nch = ceil((history + n_eff) / 8) is the sampler's chunk variant.
A1_ROWS = ([(4, 3, e, 1, 96, 8) for e in (1, 2, 3)]
           + [(4, 10, e, 1, 96, 8) for e in (1, 3, 4, 5, 9, 10)]           # nch 1 <-> 2 at h + n_eff = 8 / 9
           + [(4, 20, e, 1, 96, 8) for e in (3, 12, 13, 20)]               # nch 2 <-> 3 at 16 / 17, and the 8-chunk path
           + [(1, 10, e, 1, 96, 8) for e in (1, 10)]
           + [(4, 10, 3, 3, 192, 8),                                        # the stream stride
              (4, 10, 3, 1, 2048, 257)])                                    # the 1024-thread variant


def a1_id(row):
    h, n_max, n_eff, S, cap, B = row
    return "h%d-nmax%d-n%d-S%d-b%d" % (h, n_max, n_eff, S, B)


# the host interpreter's rows: everything but the 257-sample draw of a 2048-slot ring
A1_EMU_ROWS = [r for r in A1_ROWS if r[5] <= 8]


class HorizonAdapter(StreamsAdapter):
    """StreamsAdapter (rb_replay_create_streams; one stream is rb_replay_create's replay) plus the horizon entry points and the
    three sampler launches."""

    def __init__(self, lib, mem, capacity, history, n_max, streams=1, discount=G0, seed=7):
        super().__init__(lib, mem, capacity, history, n_max, streams, discount=discount, seed=seed)

    def set_horizon(self, n_eff, discount):
        return self.lib.rb_replay_set_horizon(self.h, int(n_eff), float(discount), self.mem.stream)

    def get_horizon(self):
        n, g = C.c_int32(-1), C.c_double(-1.0)
        L.check(self.lib, self.lib.rb_replay_get_horizon(self.h, C.byref(n), C.byref(g)))
        return int(n.value), float(g.value)

    def draw(self, batch, uu, beta=0.5, entry="plain", upd=None, job=None, stacks=True):
        """One draw with injected uniforms through rb_replay_sample ("plain"), rb_replay_update_sample ("pair": `upd` = (tree
        indices, losses) written back first) or rb_replay_sample_fused_noise ("noise": `job` from a learner)."""
        m, h = self.mem, self.history
        uu_d = m.upload(np.asarray(uu, dtype=np.float64))
        o = dict(tree_idx=m.empty((batch,), np.int64), actions=m.empty((batch,), np.int64), returns=m.empty((batch,), np.float32),
                 nonterm=m.empty((batch,), np.float32), weights=m.empty((batch,), np.float32))
        st = m.empty((batch, h, 84, 84), np.uint8) if stacks else None
        ns = m.empty((batch, h, 84, 84), np.uint8) if stacks else None
        tail = (m.ptr(o["tree_idx"]), m.ptr(st), m.ptr(ns), m.ptr(o["actions"]), m.ptr(o["returns"]), m.ptr(o["nonterm"]),
                m.ptr(o["weights"]))
        attempts = int(np.asarray(uu).shape[0])
        if entry == "plain":
            rc = self.lib.rb_replay_sample(self.h, batch, float(beta), m.ptr(uu_d), attempts, *tail, m.stream)
        elif entry == "pair":
            ti, lo = m.upload(np.asarray(upd[0], np.int64)), m.upload(np.asarray(upd[1], np.float32))
            rc = self.lib.rb_replay_update_sample(self.h, m.ptr(ti), m.ptr(lo), len(upd[0]), batch, float(beta), m.ptr(uu_d), attempts,
                                                  *tail, m.stream)
        else:
            rc = self.lib.rb_replay_sample_fused_noise(self.h, batch, float(beta), m.ptr(uu_d), attempts, *tail, C.byref(job), m.stream)
        L.check(self.lib, rc)
        m.sync()
        hdr = self.raw_header()
        assert hdr.last_status == 0, "the device sampler gave up after %d attempts" % hdr.last_attempts
        out = {k: m.download(v) for k, v in o.items()}
        out["states"] = m.download(st) if stacks else None
        out["next_states"] = m.download(ns) if stacks else None
        out["attempts"] = int(hdr.last_attempts)
        return out


def make_rows(total, S, rs, p_term=0.15, episode=None):
    """`total` transitions of S interleaved streams: per-stream episode timesteps (an episode ends with probability p_term per
    step, or after exactly `episode` steps), frames out of a pool of 64 (neighbouring ordinals never share one)."""
    assert total % S == 0
    ts, nt = np.zeros(total, np.int32), np.ones(total, np.uint8)
    t = np.zeros(S, np.int64)
    for k in range(total):
        s = k % S
        ts[k] = t[s]
        end = (t[s] + 1 == episode) if episode else (rs.random_sample() < p_term)
        if end:
            nt[k], t[s] = 0, 0
        else:
            t[s] += 1
    pool = rs.randint(0, 256, size=(64, 84, 84)).astype(np.uint8)
    pool[:, 0, 0] = np.arange(64) + 1                 # (no frame is all zero: a blanked slot cannot pass for a frame)
    return dict(ts=ts, nt=nt, pool=pool, actions=rs.randint(0, 6, total).astype(np.int32),
                rewards=rs.choice([-1.0, 0.5, 1.0, 2.0], size=total).astype(np.float32), t=t)


class Twin:
    """A device replay created with n_max and the oracles it is compared with, one per (n_eff, gamma) the scenario uses, each BUILT
    with multi_step = n_eff: all are fed the same appends and priorities."""

    def __init__(self, lib, mem, capacity, history, n_max, streams, horizons, seed=0):
        self.ad = HorizonAdapter(lib, mem, capacity, history, n_max, streams)
        self.oras = {(n, g): StreamsOracle(capacity, streams, history=history, discount=g, multi_step=n, per_stream=False)
                     for n, g in horizons}
        self.C, self.h, self.n_max, self.S = capacity, history, n_max, streams
        self.rs = np.random.RandomState(seed)
        self.ordinal = 0

    def close(self):
        self.ad.close()

    def append(self, total, **kw):
        rows = make_rows(total, self.S, self.rs, **kw)
        step = max(self.S, self.C // 2 // self.S * self.S)               # (an append takes at most `capacity` rows)
        for lo in range(0, total, step):
            sl = slice(lo, min(total, lo + step))
            frames = rows["pool"][((self.ordinal + np.arange(sl.start, sl.stop)) * 7) % 64]
            self.ad.append_batch(frames, rows["ts"][sl], rows["actions"][sl], rows["rewards"][sl], rows["nt"][sl])
            for ora in self.oras.values():
                ora.transitions.bulk_append(rows["ts"][sl], frames, rows["actions"][sl], rows["rewards"][sl], rows["nt"][sl].astype(bool))
        self.ordinal += total

    def valid(self, n):
        """Slots a draw at horizon n may use (memory.py:131 per stream, replay_sample.h)."""
        index = next(iter(self.oras.values())).transitions.index
        idx = np.arange(self.C)
        d, e = (index - idx) % self.C, (idx - index) % self.C
        return (d > n * self.S) & (d <= self.C - self.S) & (e >= self.h * self.S)

    def set_priorities(self, vals):
        tree_start = self.ad.bufs.tree_start
        vals = np.asarray(vals, np.float32)
        for lo in range(0, self.C, 1024):
            idx = np.arange(lo, min(self.C, lo + 1024)) + tree_start
            self.ad.update_leaves(idx, vals[lo:lo + 1024])
            for ora in self.oras.values():
                ora.transitions.set_leaves(idx, vals[lo:lo + 1024])

    def prioritise(self, n):
        """1 on every slot a draw at horizon n may use, 0 elsewhere (module docstring)."""
        self.set_priorities(self.valid(n).astype(np.float32))

    def expected_windows(self, ora, data_idxs):
        ring, blank = ora.window(data_idxs)
        win = np.full((len(data_idxs), self.h + self.n_max), -1, np.int32)
        win[:, :ring.shape[1]] = np.where(blank, -1, ring)
        return win

    def check(self, horizon, batch, uu, beta=0.5, label="", **draw_kw):
        """One draw on the device and on the oracle of `horizon`: everything bit for bit."""
        ora = self.oras[horizon]
        got = self.ad.draw(batch, uu, beta, **draw_kw)
        ora.priority_weight = beta
        want = ora.sample_with_uniforms(batch, uu)
        assert got["attempts"] == want["attempts"], (label, got["attempts"], want["attempts"])
        assert np.array_equal(got["tree_idx"], want["tree_idxs"]), label
        assert np.array_equal(got["actions"], want["actions"]), label
        assert np.array_equal(got["returns"].view(np.uint32), want["returns"].view(np.uint32)), (label, got["returns"], want["returns"])
        assert np.array_equal(got["nonterm"], want["nonterminals"][:, 0]), (label, got["nonterm"], want["nonterminals"][:, 0])
        assert np.array_equal(got["weights"].view(np.uint32), want["weights"].astype(np.float32).view(np.uint32)), \
            (label, got["weights"], want["weights"])
        if got["states"] is not None:
            assert np.array_equal(got["states"], want["states"]), label
            assert np.array_equal(got["next_states"], want["next_states"]), label
        win = self.ad.windows(batch)
        assert np.array_equal(win, self.expected_windows(ora, want["data_idxs"])), (label, win[:2])
        return got, want


# =============================================================================== A1. the table
def check_table_row(lib, mem, row):
    h, n_max, n_eff, S, cap, B = row
    tw = Twin(lib, mem, cap, h, n_max, S, [(n_eff, GAMMA)], seed=100 * n_max + n_eff)
    try:
        tw.append(cap + cap // 3 // S * S)
        assert tw.ad.get_horizon() == (n_max, G0)
        L.check(lib, tw.ad.set_horizon(n_eff, GAMMA))
        assert tw.ad.get_horizon() == (n_eff, GAMMA)
        assert tw.ad.bufs.window_len == h + n_max
        b = L.ReplayBuffers()
        L.check(lib, lib.rb_replay_buffers(tw.ad.h, C.byref(b)))
        assert b.window_len == h + n_max, "window_len must stay history + n_max"
        tw.prioritise(n_eff)
        blanked = tail = 0
        for k in range(3):
            got, want = tw.check((n_eff, GAMMA), B, tw.rs.random_sample((ATTEMPTS, B)), label="%s draw %d" % (a1_id(row), k))
            win = tw.ad.windows(B)
            blanked += int((win[:, :h + n_eff] < 0).sum())
            tail += int((win[:, h + n_eff:] != -1).sum())
        assert blanked > 0, "the scenario must blank slots"
        assert tail == 0
    finally:
        tw.close()


# =============================================================================== uniforms that land on chosen slots
def stratum_hits(ora, batch, i, K=2048):
    """{data index: a unit uniform of stratum i that the oracle's tree search maps to it} over a grid of K points (the sampler's
    own arithmetic, memory.py:125-130)."""
    tr = ora.transitions
    seg = np.float32(tr.total()) / np.float32(batch)
    start = np.int64(i) * np.float64(seg)
    us = (np.arange(K) + 0.5) / K
    samples = (0.0 + np.float64(seg) * us) + start
    _p, idxs, _t = tr.find(samples)
    return {int(d): float(u) for d, u in zip(idxs[::-1], us[::-1])}


def uniforms_for(ora, batch, wanted, fallback):
    """One attempt's uniforms: each set of `wanted` (a list of sets of data indices) is hit by a stratum of its own, the other
    strata land in `fallback`.  Returns (u [batch], the stratum of each wanted set)."""
    hits = [stratum_hits(ora, batch, i) for i in range(batch)]
    u, used, where = np.zeros(batch), set(), []
    for want in wanted:
        found = next(((i, d) for i in range(batch) if i not in used for d in sorted(hits[i]) if d in want), None)
        assert found is not None, "no free stratum reaches %s" % sorted(want)
        i, d = found
        u[i] = hits[i][d]
        used.add(i)
        where.append(i)
    for i in range(batch):
        if i not in used:
            d = next(d for d in sorted(hits[i]) if d in fallback)
            u[i] = hits[i][d]
    return u, where


# =============================================================================== A2. episode ends against the horizon
def check_episode_ends(lib, mem, h=4, n_max=10, n_eff=3, cap=96, B=8):
    """One stream, an episode end every 14 transitions (the window is 14 slots: never two ends in one), and uniforms that put a
    sample exactly k transitions in front of a terminal transition for k in {n_eff - 1, n_eff, n_eff + 1, n_max - 1}.  What the
    reference does with n = n_eff (memory.py:111-145), asserted on the oracle ALONE before the device is looked at:
      k = n_eff - 1   inside the horizon: the episode's successor sits in window slot h + n_eff - 1, which is blanked — nonterminal 0
                      and a blank last frame of the next stack;
      k = n_eff       the nonterminal IS the flag of the transition at idx + n_eff (memory.py:145), so it reads 0; the return and the
                      next stack are whole;
      k = n_eff + 1, n_max - 1   beyond the horizon: return, nonterminal (1) and next stack untouched — while a replay at n_max blanks
                      the tail of the same window, zeroes the nonterminal and cuts the return: an implementation that only rescaled
                      the returns of the n_max window fails here."""
    tw = Twin(lib, mem, cap, h, n_max, 1, [(n_eff, GAMMA), (n_max, GAMMA)], seed=2)
    try:
        tw.append(cap + 30, episode=14)
        L.check(lib, tw.ad.set_horizon(n_eff, GAMMA))
        tw.prioritise(n_eff)
        ora, ora_max = tw.oras[(n_eff, GAMMA)], tw.oras[(n_max, GAMMA)]
        tr = ora.transitions
        valid = tw.valid(n_eff) & tw.valid(n_max)        # (the n_max oracle is asked about the same samples below)
        ks = (n_eff - 1, n_eff, n_eff + 1, n_max - 1)
        wanted = [{int(i) for i in np.flatnonzero(valid) if not tr.nonterminal[(i + k) % cap]} for k in ks]
        u, where = uniforms_for(ora, B, wanted, set(np.flatnonzero(valid).tolist()))
        uu = np.stack([u] * 2)
        # ---- the oracle alone
        ora.priority_weight = 0.5
        want = ora.sample_with_uniforms(B, uu)
        assert want["attempts"] == 1
        ring_max, blank_max = ora_max.window(want["data_idxs"])
        sc_max = ora_max.batch_scalars(want["data_idxs"], want["probs"])
        kinds = {"inside": 0, "at": 0, "beyond": 0}
        for k, i in zip(ks, where):
            d = int(want["data_idxs"][i])
            assert not tr.nonterminal[(d + k) % cap]
            rewards = tr.reward[(d + np.arange(n_eff)) % cap]
            full = np.float32(0)
            for j in range(n_eff):
                full = full + rewards[j] * ora.n_step_scaling[j]
            whole = want["next_states"][i].reshape(h, -1).any(axis=1).all()
            if k < n_eff:
                kinds["inside"] += 1
                assert want["nonterminals"][i, 0] == 0.0 and not want["next_states"][i, -1].any()
            elif k == n_eff:
                kinds["at"] += 1
                assert want["nonterminals"][i, 0] == 0.0 and whole and want["returns"][i] == full
            else:
                kinds["beyond"] += 1
                assert want["nonterminals"][i, 0] == 1.0 and whole and want["returns"][i] == full
                # the same sample at n_max: the window's tail blanked, nonterminal 0
                assert sc_max["nonterminals"][i, 0] == 0.0 and blank_max[i, -1]
        assert kinds == {"inside": 1, "at": 1, "beyond": 2}, kinds
        # ---- the device
        tw.check((n_eff, GAMMA), B, uu, label="episode ends")
    finally:
        tw.close()


# =============================================================================== A3. the write-head rule
def check_write_head(lib, guarded_mem, h=4, n_max=10, n_eff=3, S=1, cap=96, B=8):
    """Ring full; leaves at distance d from the write head with n_eff S < d <= n_max S are legal at n_eff and illegal at n_max.
    Draw 1 lands on such leaves with its FIRST attempt: the oracle at n_eff accepts it at once and so must the device.  Draw 2 puts
    the leaf AT distance n_eff S in front (rejected at either horizon: memory.py:131 is a strict >) and the same leaves behind it:
    accepted as the second attempt.  The gather of those rows reads slots [n_eff, n_eff + h) of the window table, never its -1 tail:
    the stacks equal the oracle's, and the canaries round every caller buffer (tests/guarded_mem.py) are intact.  At n_max the
    same uniforms find no legal batch.  S = 3 runs the rule per stream."""
    tw = Twin(lib, guarded_mem, cap, h, n_max, S, [(n_eff, GAMMA), (n_max, GAMMA)], seed=3)
    try:
        tw.append(cap + cap // 3 // S * S, p_term=0.05)
        L.check(lib, tw.ad.set_horizon(n_eff, GAMMA))
        ora = tw.oras[(n_eff, GAMMA)]
        index = ora.transitions.index
        assert ora.transitions.full
        edge = (index - n_eff * S) % cap                                   # d == n_eff S: not legal
        near = [(index - d) % cap for d in range(n_eff * S + 1, n_max * S + 1)]
        vals = tw.valid(n_eff).astype(np.float32)
        assert all(vals[d] == 1 for d in near) and vals[edge] == 0 and not tw.valid(n_max)[near].any()
        vals[edge] = 1
        tw.set_priorities(vals)
        legal = set(np.flatnonzero(tw.valid(n_eff)).tolist())
        wanted = [{int(near[0])}, {int(near[-1])}] if S == 1 else [set(int(d) for d in near)]
        u1, _ = uniforms_for(ora, B, [{int(edge)}], legal)
        u2, where = uniforms_for(ora, B, wanted, legal)
        got, want = tw.check((n_eff, GAMMA), B, np.stack([u2, u2]), label="write head, first attempt")
        assert want["attempts"] == 1 and got["attempts"] == 1
        for i, w in zip(where, wanted):
            assert int(want["data_idxs"][i]) in w
        uu = np.stack([u1, u2, u2])
        got, want = tw.check((n_eff, GAMMA), B, uu, label="write head, behind the edge leaf")
        assert want["attempts"] == 2
        try:                                                               # at n_max the same uniforms find no legal batch
            tw.oras[(n_max, GAMMA)].draw_indices(B, uu)
            raise AssertionError("the oracle at n_max accepted a leaf inside its exclusion zone")
        except RuntimeError:
            pass
        n, bad = guarded_mem.check()
        assert n >= 8 and not bad, bad
    finally:
        tw.close()


def check_random_priorities(lib, mem, h=4, n_max=10, n_eff=3, cap=96, B=8):
    """Beside the table: random priorities on EVERY slot, the write head's exclusion zone included, so that the rejection loop runs
    (some draw must need more than one attempt) and the importance weights differ from sample to sample.  Indices, attempts,
    actions, returns, nonterminals, stacks and the window table exact; the weights at helpers.F32_ULP_RTOL, the bound the existing
    parity tests give a float32 power (the horizon does not enter them)."""
    from helpers import F32_ULP_RTOL
    tw = Twin(lib, mem, cap, h, n_max, 1, [(n_eff, GAMMA)], seed=8)
    try:
        tw.append(cap + 30)
        L.check(lib, tw.ad.set_horizon(n_eff, GAMMA))
        tw.set_priorities(tw.rs.random_sample(cap) * 2 + 0.25)
        ora = tw.oras[(n_eff, GAMMA)]
        ora.priority_weight = 0.5
        most = 0
        for k in range(6):
            uu = tw.rs.random_sample((32, B))
            got = tw.ad.draw(B, uu, 0.5)
            want = ora.sample_with_uniforms(B, uu)
            most = max(most, want["attempts"])
            assert got["attempts"] == want["attempts"] and np.array_equal(got["tree_idx"], want["tree_idxs"]), k
            assert np.array_equal(got["actions"], want["actions"]) and np.array_equal(got["nonterm"], want["nonterminals"][:, 0]), k
            assert np.array_equal(got["returns"].view(np.uint32), want["returns"].view(np.uint32)), k
            assert np.array_equal(got["states"], want["states"]) and np.array_equal(got["next_states"], want["next_states"]), k
            assert np.array_equal(tw.ad.windows(B), tw.expected_windows(ora, want["data_idxs"])), k
            np.testing.assert_allclose(got["weights"], want["weights"], rtol=F32_ULP_RTOL)
            assert len(np.unique(want["weights"])) > 1
        assert most >= 2, "the scenario must reject a draw"
    finally:
        tw.close()


# =============================================================================== A4. change on a live replay
def check_live_change(lib, mem, h=4, n_max=10, cap=96, B=8):
    """sample -> set_horizon(3, 0.997) -> sample -> set_horizon(10, 0.97) -> sample with appends in between, each batch equal to
    the oracle of the horizon then in force: the first through rb_replay_sample, the second through the pair launch
    rb_replay_update_sample (writing back the first batch at loss 1), the third through rb_replay_sample_fused_noise; then horizon
    3 again and the shifted gather (pad 4, injected shifts) of a draw with NULL stacks."""
    lo, hi = (3, GAMMA), (n_max, G0)
    tw = Twin(lib, mem, cap, h, n_max, 1, [lo, hi], seed=4)
    learner = make_learner(lib, mem, "horizon-job", dict(scenarios.LEARN_CONFIGS["k10"], multi_step=n_max))
    try:
        job = L.NoiseJob()
        L.check(lib, lib.rb_learner_noise_job(learner.h, 1, C.byref(job)))
        tw.append(cap + 30)
        tw.prioritise(n_max)
        got, want = tw.check(hi, B, tw.rs.random_sample((ATTEMPTS, B)), label="live: creation horizon")
        tw.append(12)
        L.check(lib, tw.ad.set_horizon(*lo))
        tw.prioritise(3)
        ones = np.ones(B, np.float32)
        for ora in tw.oras.values():
            ora.update_priorities(want["tree_idxs"], ones)
        tw.check(lo, B, tw.rs.random_sample((ATTEMPTS, B)), label="live: pair launch at 3", entry="pair", upd=(want["tree_idxs"], ones))
        tw.append(12)
        L.check(lib, tw.ad.set_horizon(*hi))
        tw.prioritise(n_max)
        tw.check(hi, B, tw.rs.random_sample((ATTEMPTS, B)), label="live: fused noise at 10", entry="noise", job=job)
        # ---- the shifted gather at 3 of 10
        L.check(lib, tw.ad.set_horizon(*lo))
        tw.prioritise(3)
        got, want = tw.check(lo, B, tw.rs.random_sample((ATTEMPTS, B)), label="live: NULL stacks at 3", stacks=False)
        m = tw.ad.mem
        shifts = tw.rs.randint(-4, 5, size=(B, 2, 2)).astype(np.int8)
        st, ns = m.empty((B, h, 84, 84), np.uint8), m.empty((B, h, 84, 84), np.uint8)
        sin, sout = m.upload(shifts.view(np.uint8)), m.upload(np.full((B, 2, 2), 0x55, np.uint8))
        L.check(lib, lib.rb_replay_gather_shifted(tw.ad.h, B, 4, 0, m.ptr(sin), m.ptr(st), m.ptr(ns), m.ptr(sout), m.stream))
        m.sync()
        want_s, want_n = SO.shift_batch(want["states"], want["next_states"], shifts)
        assert np.array_equal(m.download(sout).view(np.int8), shifts)
        assert np.array_equal(m.download(st), want_s) and np.array_equal(m.download(ns), want_n)
        assert (want["next_states"].reshape(B, -1) != want["states"].reshape(B, -1)).any()
    finally:
        learner.close()
        tw.close()


# =============================================================================== A6. refusals
def check_refusals(lib, mem, h=4, n_max=10, cap=96, B=8):
    """n_eff = 0, n_eff = n_max + 1, discount 0 and discount 1.5 (and NaN, and a NULL handle): an error code and a message that
    names the entry point and the argument; the horizon is unchanged and the replay draws as before."""
    tw = Twin(lib, mem, cap, h, n_max, 1, [(3, GAMMA)], seed=6)
    try:
        tw.append(cap + 30)
        L.check(lib, tw.ad.set_horizon(3, GAMMA))
        tw.prioritise(3)
        for n, g, word in ((0, 0.99, "n_eff"), (n_max + 1, 0.99, "n_eff"), (3, 0.0, "discount"), (3, 1.5, "discount"),
                           (3, float("nan"), "discount")):
            rc = tw.ad.set_horizon(n, g)
            msg = lib.rb_last_error().decode()
            assert rc < 0 and "rb_replay_set_horizon" in msg and word in msg, (n, g, rc, msg)
            assert tw.ad.get_horizon() == (3, GAMMA)
        assert lib.rb_replay_set_horizon(None, 3, 0.99, mem.stream) < 0 and "handle" in lib.rb_last_error().decode()
        assert lib.rb_replay_get_horizon(tw.ad.h, None, None) < 0
        tw.check((3, GAMMA), B, tw.rs.random_sample((ATTEMPTS, B)), label="after the refusals")
        L.check(lib, tw.ad.set_horizon(n_max, 1.0))          # the limits themselves pass
        L.check(lib, tw.ad.set_horizon(1, GAMMA))
    finally:
        tw.close()


# =============================================================================== the learner's entry points
def learner_horizon(lib, ad):
    n, g = C.c_int32(-1), C.c_double(-1.0)
    L.check(lib, lib.rb_learner_get_horizon(ad.h, C.byref(n), C.byref(g)))
    return int(n.value), float(g.value)


def check_learner_refusals(lib, mem):
    ad = make_learner(lib, mem, "horizon-refusals", dict(scenarios.LEARN_CONFIGS["k10"], multi_step=10, discount=G0))
    try:
        assert learner_horizon(lib, ad) == (10, G0)
        for n, g, word in ((0, 0.99, "n_eff"), (11, 0.99, "n_eff"), (3, 0.0, "discount"), (3, 1.5, "discount")):
            rc = lib.rb_learner_set_horizon(ad.h, n, g)
            msg = lib.rb_last_error().decode()
            assert rc < 0 and "rb_learner_set_horizon" in msg and word in msg, (n, g, rc, msg)
            assert learner_horizon(lib, ad) == (10, G0)
        assert lib.rb_learner_set_horizon(None, 3, 0.99) < 0
        L.check(lib, lib.rb_learner_set_horizon(ad.h, 3, GAMMA))
        assert learner_horizon(lib, ad) == (3, GAMMA)
    finally:
        ad.close()


# =============================================================================== B. the learn step
HORIZON_STEPS = ((3, 0.997), (7, 0.98))
# row: (configuration, seed, the oracle's hidden ReLU margin of step 0 / 1 as `PYTHONPATH=. python tests/horizon_scenarios.py` printed them, CPU only)
LEARN_ROWS = {
    "dataeff-b4-h32": (dict(architecture="data-efficient", hidden=32, actions=6, atoms=51, batch=4, multi_step=10, discount=G0,
                            history=4, v_min=-10.0, v_max=10.0), 0, (1.720e-04, 1.638e-04)),
    "canonical-b32-h512": (dict(architecture="canonical", hidden=512, actions=6, atoms=51, batch=32, multi_step=10, discount=G0,
                                history=4, v_min=-10.0, v_max=10.0), 0, (2.179e-06, 4.254e-07)),
}
SPARE = 2.5


class HorizonOracleRun(OracleRun):
    """learn_steps.OracleRun with the step's (n, gamma) in the oracle's Config."""

    def __init__(self, inp, cfgd):
        super().__init__(inp)
        self.cfgd = cfgd

    def step(self, k, **kw):
        n, g = HORIZON_STEPS[k]
        self.inp["cfg"] = O.Config(**dict(self.cfgd, multi_step=n, discount=g))
        return super().step(k, **kw)


def oracle_margins(row, seed):
    cfgd = LEARN_ROWS[row][0]
    run = HorizonOracleRun(two_step_inputs(cfgd, seed), cfgd)
    return tuple(float(run.step(k)["want"]["hidden_relu_margin"]) for k in range(2))


def check_learn(lib, mem, row, where="hip"):
    """Two learn steps through rb_learner_learn (gathered stacks) with the horizon changed before each, against the oracle."""
    cfgd, seed, _margins = LEARN_ROWS[row]
    inp = two_step_inputs(cfgd, seed)
    B, Z = cfgd["batch"], cfgd["atoms"]
    what = "%s/%s" % (where, row)
    ad = make_learner(lib, mem, "horizon-" + row, cfgd)
    try:
        ad.load(inp["online"], inp["target"])
        stepper = HorizonOracleRun(inp, cfgd)
        got_t, want_t = {}, {}
        for k, st in enumerate(inp["steps"]):
            L.check(lib, lib.rb_learner_set_horizon(ad.h, *HORIZON_STEPS[k]))
            ad.reset_noise_online(st["raw_on"])
            got = ad.learn_step(st["batch"], st["raw_tg"])
            conv_masks = [ad.debug(6 + i, shp, np.float32) > 0 for i, shp in enumerate(conv_shapes(inp["cfg"], B))]
            o = stepper.step(k, conv_masks=conv_masks)
            want = o["want"]
            print("%s step %d: hidden ReLU margin %.3e; conv ReLU decisions that differ from the oracle's own %s"
                  % (what, k, want["hidden_relu_margin"], ["%d %.1e %.1e" % f for f in want["conv_flips"]]))
            assert want["hidden_relu_margin"] >= RELU_MARGIN, "%s: ill-conditioned seed at step %d (%.3e)" % (what, k, want["hidden_relu_margin"])
            assert all(ratio < 1.0 for _n, _a, ratio in want["conv_flips"]), (what, k, want["conv_flips"])
            got_t["s%d_loss" % k], want_t["s%d_loss" % k] = got["loss"], want["loss"]
            got_t["s%d_grad_norm" % k], want_t["s%d_grad_norm" % k] = np.float32(got["grad_norm"]), np.float32(o["total"])
            for name in o["clipped"]:
                got_t["s%d_grad/%s" % (k, name)], want_t["s%d_grad/%s" % (k, name)] = got["grads"][name], o["clipped"][name]
            for name, p in ad.params().items():
                got_t["s%d_param/%s" % (k, name)], want_t["s%d_param/%s" % (k, name)] = p, o["params"][name]
            np.testing.assert_allclose(ad.debug(1, (B, Z), np.float32), want["m"], rtol=1e-4, atol=1e-6,
                                       err_msg="%s: projected m of step %d" % (what, k))
        assert_learn_trace_matches(got_t, want_t, label=what)
    finally:
        ad.close()


# =============================================================================== train_step: mismatch, early draw, twin
def _ts_config(n_max=10):
    return dict(scenarios.LEARN_CONFIGS["k10"], multi_step=n_max, discount=G0)


class _TsConfig:
    """ts_scenarios.ts_build / ts_args look their configuration up by name."""
    name = "_horizon_ts"

    def __enter__(self):
        scenarios.LEARN_CONFIGS[self.name] = _ts_config()
        return self.name

    def __exit__(self, *exc):
        del scenarios.LEARN_CONFIGS[self.name]


def _set_both(lib, h, n, g):
    mem, rp, ad, o, job = h
    L.check(lib, lib.rb_replay_set_horizon(rp.h, n, g, mem.stream))
    L.check(lib, lib.rb_learner_set_horizon(ad.h, n, g))


def check_train_step_mismatch(lib, Mem):
    """The replay at 3, the learner at 10: rb_learner_train_step returns an error that names both pairs and launches nothing (batch
    buffers, parameters and the replay's header keep their bytes); with the learner set to 3 as well the call goes through."""
    import ts_scenarios as TS
    with _TsConfig() as name:
        h = TS.ts_build(lib, Mem, name)
        mem, rp, ad, o, job = h
        try:
            L.check(lib, lib.rb_replay_set_horizon(rp.h, 3, GAMMA, mem.stream))
            mem.sync()
            before, hdr0 = TS.ts_snapshot(mem, rp, ad, o), bytes(rp.raw_header())
            ts = TS.ts_args(name, mem, rp, ad, o, job, 0.4, 1)
            rc = lib.rb_learner_train_step(ad.h, C.byref(ts), mem.stream)
            msg = lib.rb_last_error().decode()
            assert rc < 0 and "rb_learner_train_step" in msg and "horizon" in msg and "(3," in msg and "(10," in msg, (rc, msg)
            after = TS.ts_snapshot(mem, rp, ad, o)
            for k in before:
                assert np.array_equal(before[k], after[k]), k
            assert bytes(rp.raw_header()) == hdr0
            L.check(lib, lib.rb_learner_set_horizon(ad.h, 3, 0.99))           # the horizon alone is not enough
            assert lib.rb_learner_train_step(ad.h, C.byref(ts), mem.stream) < 0
            L.check(lib, lib.rb_learner_set_horizon(ad.h, 3, GAMMA))
            L.check(lib, lib.rb_learner_train_step(ad.h, C.byref(ts), mem.stream))
            mem.sync()
            assert rp.raw_header().last_status == 0
        finally:
            ad.close(); rp.close()


def _oracle_scalars(mem, rp, n, g, tree_idx):
    """Returns, nonterminals and window rows of the batch at `tree_idx` from the device's own columns, by the oracle at (n, g)."""
    from oracle.replay_oracle import ReplayOracle
    cap, b = rp.capacity, rp.bufs
    ora = ReplayOracle(cap, history=rp.history, discount=g, multi_step=n)
    tr = ora.transitions
    tr.timestep = mem.view(b.timestep_dev, (cap,), np.int32)
    tr.action = mem.view(b.action_dev, (cap,), np.int32)
    tr.reward = mem.view(b.reward_dev, (cap,), np.float32)
    tr.nonterminal = mem.view(b.nonterminal_dev, (cap,), np.uint8).astype(bool)
    tr.tree = rp.tree()
    idxs = np.asarray(tree_idx) - tr.tree_start
    with np.errstate(all="ignore"):
        sc = ora.batch_scalars(idxs, np.ones(len(idxs), np.float32))
    ring, blank = ora.window(idxs)
    return sc["returns"], sc["nonterminals"][:, 0], np.where(blank, -1, ring)


def check_train_step(lib, Mem, monkeypatch, spec):
    """rb_learner_train_step under a changing horizon against a twin that issues the step's three entry points itself
    (rb_replay_sample_fused_noise, rb_learner_learn_windows, rb_learner_clip_adam), bit for bit after every call: two calls at the
    creation horizon, set_horizon(3, 0.997) on replay and learner, two more calls.  spec = True runs the first handle under RB_OPTS
    spec_draw=1: call 2 leaves a tentative draw made at horizon 10 in flight, which call 3 must discard (A5) — its batch is the
    twin's, its returns, nonterminals and window rows are the oracle's at horizon 3 on the device's own columns, the table's tail is
    -1, and rb_replay_expired_waits stays 0."""
    import ts_scenarios as TS
    hy = scenarios.LEARN_HYPER
    with _TsConfig() as name:
        B = scenarios.LEARN_CONFIGS[name]["batch"]
        monkeypatch.setenv("RB_OPTS", "spec_draw=1" if spec else "spec_draw=0")
        h1 = TS.ts_build(lib, Mem, name)
        monkeypatch.setenv("RB_OPTS", "spec_draw=0")
        h2 = TS.ts_build(lib, Mem, name)
        try:
            for step in range(1, 5):
                if step == 3:
                    if spec:       # (a tentative draw IS in flight: the speculating handle's buffers already hold another batch)
                        h1[0].sync()
                        assert not np.array_equal(h1[0].download(h1[3]["tree_idx"]), h2[0].download(h2[3]["tree_idx"])), \
                            "the scenario needs a tentative draw in flight"
                    for h in (h1, h2):
                        _set_both(lib, h, 3, GAMMA)
                mem, rp, ad, o, job = h1
                ts = TS.ts_args(name, mem, rp, ad, o, job, 0.4, step)
                L.check(lib, lib.rb_learner_train_step(ad.h, C.byref(ts), mem.stream))
                mem, rp, ad, o, job = h2
                L.check(lib, lib.rb_replay_sample_fused_noise(rp.h, B, 0.4, None, 64, mem.ptr(o["tree_idx"]), None, None,
                                                             mem.ptr(o["actions"]), mem.ptr(o["returns"]), mem.ptr(o["nonterm"]),
                                                             mem.ptr(o["weights"]), C.byref(job), mem.stream))
                L.check(lib, lib.rb_learner_learn_windows(ad.h, rp.bufs.frames_dev, rp.bufs.window_dev, rp.bufs.window_len,
                                                          mem.ptr(o["actions"]), mem.ptr(o["returns"]), mem.ptr(o["nonterm"]),
                                                          mem.ptr(o["weights"]), mem.ptr(o["loss"]), mem.stream))
                L.check(lib, lib.rb_learner_clip_adam(ad.h, hy["norm_clip"], mem.ptr(ad.adam_m), mem.ptr(ad.adam_v), hy["lr"], 0.9, 0.999,
                                                      hy["adam_eps"], step, mem.ptr(o["norm"]), mem.stream))
                if step == 3:
                    # the twin's batch of call 3 by the oracle at horizon 3 (before the handles run on: buffers are reused)
                    mem.sync()
                    n_max = scenarios.LEARN_CONFIGS[name]["multi_step"]
                    idx = mem.download(o["tree_idx"]).copy()
                    R, nt, win = _oracle_scalars(mem, rp, 3, GAMMA, idx)
                    assert np.array_equal(mem.download(o["returns"]).view(np.uint32), R.view(np.uint32))
                    assert np.array_equal(mem.download(o["nonterm"]), nt)
                    table = mem.view(rp.bufs.window_dev, (B, rp.history + n_max), np.int32)
                    assert np.array_equal(table[:, :rp.history + 3], win) and (table[:, rp.history + 3:] == -1).all()
                    R10, _nt10, _w = _oracle_scalars(mem, rp, n_max, G0, idx)
                    assert not np.array_equal(R, R10), "the scenario needs returns that tell the horizons apart"
                a, b = TS.ts_snapshot(*h1[:4]), TS.ts_snapshot(*h2[:4])
                # (under spec_draw the calls that launch an early pair — the second of each run of like calls — leave the NEXT
                # call's tentative batch in the speculating handle's buffers; call 3, the one that must discard it, compares whole)
                ahead = ("idx", "w") if spec and step in (2, 4) else ()
                for k in a:
                    assert k in ahead or np.array_equal(a[k], b[k]), ("call %d" % step, k)
            e = C.c_int64(-1)
            L.check(lib, lib.rb_replay_expired_waits(h1[1].h, C.byref(e)))
            assert e.value == 0
        finally:
            for (mem, rp, ad, o, job) in (h1, h2):
                ad.close(); rp.close()


if __name__ == "__main__":       # the seed search of LEARN_ROWS (CPU, oracle only)
    for row in LEARN_ROWS:
        for seed in range(14):
            margins = oracle_margins(row, seed)
            print(row, seed, "%.3e %.3e" % margins, flush=True)
            if min(margins) >= SPARE * RELU_MARGIN:
                break
