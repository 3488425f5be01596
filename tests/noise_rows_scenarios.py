"""Checks of the per-row-noise act path (rb_learner_noise_rows, rb_learner_act_batch_rows) shared by the host-interpreter tests
(test_noise_rows_emu.py) and the device tests (test_noise_rows_gpu.py): the same code drives either build through the C ABI.

The oracle is oracle.learner_oracle.act(cfg, params, make_noise(cfg, raw[i]), state[i]), one row at a time: the reference's own
rounding order (W = mu + sigma * (eps_out eps_in^T) formed per row, then contracted).  The library contracts mu and sigma
separately (csrc/noisy_rows.h), so q agrees within the act-path tolerance, not to the bit."""
import ctypes as C

import numpy as np

import scenarios
from cabi_adapter import CAbiLearnAdapter
from eval_scenarios import bits, varied_states
from oracle import learner_oracle as O
from rainbow_amd import _lib as L

RTOL, ATOL = 2e-5, 1e-6          # the project's act-path tolerance for q against the oracle (test_learner_gpu.py)
MIN_MARGIN = 1e-3                # every row's top-two q margin in the oracle: far above the tolerance, so the action is decided
CFG2 = "cfg2-canonical-h512-b32-a6"
EXTRA_SHAPES = {CFG2: dict(architecture="canonical", hidden=512, actions=6, atoms=51, batch=32, multi_step=3, discount=0.99,
                           history=4, v_min=-10.0, v_max=10.0)}      # the BASELINE cfg-2 network


def shape_of(name):
    return EXTRA_SHAPES[name] if name in EXTRA_SHAPES else scenarios.LEARN_CONFIGS[name]


def scaled_params(cfg):
    """eval_scenarios.eval_learner's parameters: seed 31, noisy-linear means x 8 (with the plain initialisation the advantage
    biases decide every greedy action and all states get the same one)."""
    return {k: (v * 8.0 if k.startswith("fc_") and k.endswith("weight_mu") else v) for k, v in O.init_params(cfg, 31).items()}


def make_learner(lib, mem, name, params):
    added = name not in scenarios.LEARN_CONFIGS
    if added:
        scenarios.LEARN_CONFIGS[name] = EXTRA_SHAPES[name]
    try:
        ad = CAbiLearnAdapter(lib, mem, name)
    finally:
        if added:
            del scenarios.LEARN_CONFIGS[name]
    ad.load(params, params)
    return ad


def raw_normals(seed, n, draws):
    return np.random.RandomState(seed).randn(n, draws).astype(np.float32)


# ------------------------------------------------------------------------------- the oracle, once per (shape, rows, seed)
_ORACLE = {}


def oracle_rows(name, n, seed):
    """Per row i: the oracle's (action, q) under ITS noise and under row 0's noise (what an implementation that shares one
    noise row computes), and the row's top-two q margin under its own noise.  Cached for the process."""
    key = (name, n, seed)
    if key not in _ORACLE:
        import torch
        cfg = O.Config(**shape_of(name))
        params = scaled_params(cfg)
        states = varied_states(n, cfg.history)
        raw = raw_normals(seed, n, O.noise_draw_count(cfg))
        p = {k: torch.as_tensor(np.ascontiguousarray(v)) for k, v in params.items()}
        a, q, margin = np.zeros(n, np.int64), np.zeros(n, np.float32), np.zeros(n, np.float64)
        for i in range(n):
            noise = O.make_noise(cfg, raw[i])
            a[i], q[i] = O.act(cfg, params, noise, states[i])
            with torch.no_grad():
                qs = (O.forward(cfg, p, noise, torch.as_tensor(states[i:i + 1])) * O.support(cfg)).sum(2)[0].numpy()
            top = np.sort(qs.astype(np.float64))
            margin[i] = top[-1] - top[-2]
        with torch.no_grad():
            qs0 = (O.forward(cfg, p, O.make_noise(cfg, raw[0]), torch.as_tensor(states)) * O.support(cfg)).sum(2).numpy()
        _ORACLE[key] = dict(a=a, q=q, margin=margin, a_shared=qs0.argmax(1).astype(np.int64), q_shared=qs0.max(1).astype(np.float32))
    return _ORACLE[key]


def preconditions_hold(ora):
    return bool(ora["margin"].min() >= MIN_MARGIN and (ora["a"] != ora["a_shared"]).any()
                and np.abs(ora["q"] - ora["q_shared"]).max() > 0.01)


def pick_noise_seed(name, n):
    """The first seed (from 6, the one the arithmetic was first checked with) whose ORACLE rows meet the parity test's
    preconditions over all n rows: every top-two margin >= 1e-3, and per-row noise differs from shared noise in at least one
    action and by more than 0.01 in some q.  Decided on the CPU, from the oracle alone; no row is skipped."""
    for seed in range(6, 60):
        if preconditions_hold(oracle_rows(name, n, seed)):
            return seed
    raise AssertionError("no noise seed in [6, 60) meets the preconditions for %s at %d rows" % (name, n))


# ------------------------------------------------------------------------------- one learner and its rows on the device
class RowsContext:
    """One learner of shape `name` with eval_learner-style parameters, n_max varied states and one block of raw normals per
    row; noise rows [n_max][n_noise] filled ONCE through rb_learner_noise_rows with the injected normals."""

    def __init__(self, lib, mem, name, n_max):
        self.lib, self.mem, self.name, self.n_max = lib, mem, name, n_max
        self.c = shape_of(name)
        self.cfg = O.Config(**self.c)
        self.seed = pick_noise_seed(name, n_max)
        self.ora = oracle_rows(name, n_max, self.seed)
        self.params = scaled_params(self.cfg)
        self.ad = make_learner(lib, mem, name, self.params)
        self.n_noise = self.ad.n_noise
        self.draws = O.noise_draw_count(self.cfg)
        assert self.draws == lib.rb_learner_noise_draws(C.byref(self.ad.cfg))
        self.states_np = varied_states(n_max, self.cfg.history)
        self.raw_np = raw_normals(self.seed, n_max, self.draws)
        self.states = mem.upload(self.states_np)
        self.raw = mem.upload(self.raw_np)
        self.noise = mem.empty((n_max, self.n_noise), np.float32)
        self.fill(self.noise, n_max, raw=self.raw)

    def close(self):
        self.ad.close()

    def fill(self, buf, rows, row0=0, seed=0, rnd=0, raw=None, offset=0):
        m = self.mem
        L.check(self.lib, self.lib.rb_learner_noise_rows(self.ad.h, rows, row0, seed, rnd, m.ptr(raw) if raw is not None else None,
                                                         m.ptr(buf) + 4 * offset, m.stream))
        m.sync()

    def generate(self, rows, row0, seed, rnd):
        buf = self.mem.empty((rows, self.n_noise), np.float32)
        self.fill(buf, rows, row0, seed, rnd)
        return self.mem.download(buf)

    def act_rows(self, n, states=None, noise=None):
        m = self.mem
        a, q = m.upload(np.full(n, -3, dtype=np.int32)), m.empty((n,), np.float32)
        L.check(self.lib, self.lib.rb_learner_act_batch_rows(self.ad.h, m.ptr(self.states if states is None else states), n,
                                                             m.ptr(self.noise if noise is None else noise), m.ptr(a), m.ptr(q), m.stream))
        m.sync()
        return m.download(a).astype(np.int64), m.download(q).copy()

    def act_shared(self, n, noisy):
        m = self.mem
        a, q = m.empty((n,), np.int32), m.empty((n,), np.float32)
        L.check(self.lib, self.lib.rb_learner_act_batch(self.ad.h, m.ptr(self.states), n, noisy, m.ptr(a), m.ptr(q), m.stream))
        m.sync()
        return m.download(a).astype(np.int64), m.download(q).copy()

    def live_mask(self):
        from cabi_adapter import query_layout
        live = np.zeros(self.n_noise, dtype=bool)
        for _name, (off, shp) in query_layout(self.lib, self.ad.cfg, self.lib.rb_learner_noise_layout).items():
            live[off:off + shp[0]] = True
        return live


def close_q(got, want):
    return np.allclose(got, want, rtol=RTOL, atol=ATOL)


def q_error_share(got, want):
    """|got - want| as a share of the tolerance (<= 1 passes)."""
    want = np.asarray(want, dtype=np.float64)
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / (ATOL + RTOL * np.abs(want))).max())


# =============================================================================== 1. parity
def check_context_preconditions(ctx):
    """From the oracle alone, over all rows of the context: margins, and per-row noise is not shared noise."""
    ora = ctx.ora
    assert ora["margin"].min() >= MIN_MARGIN, ora["margin"].min()
    assert (ora["a"] != ora["a_shared"]).any(), "per-row and shared-noise oracle pick the same action in every row"
    assert np.abs(ora["q"] - ora["q_shared"]).max() > 0.01


def check_parity(ctx, n):
    """Rows [0, n) of the context through rb_learner_act_batch_rows: every action is the oracle's, q within the act tolerance."""
    ora = ctx.ora
    check_context_preconditions(ctx)
    assert ora["margin"][:n].min() >= MIN_MARGIN
    if n >= 2:
        assert np.abs(ora["q"][:n] - ora["q_shared"][:n]).max() > 0.01      # a kernel that shares row 0's noise misses q
    a, q = ctx.act_rows(n)
    print("noise_rows parity %s n=%d seed=%d: worst q error %.3f of the tolerance, smallest margin %.2e, %d of %d actions differ from "
          "shared noise" % (ctx.name, n, ctx.seed, q_error_share(q, ora["q"][:n]), ora["margin"][:n].min(),
                            int((ora["a"][:n] != ora["a_shared"][:n]).sum()), n))
    assert np.array_equal(a, ora["a"][:n]), (a.tolist(), ora["a"][:n].tolist())
    assert close_q(q, ora["q"][:n]), q_error_share(q, ora["q"][:n])


# =============================================================================== 2. consistency with the shared-noise path
def check_consistency(ctx, n):
    """The same noise row n times = rb_learner_act_batch(noisy = 1) after rb_learner_reset_noise with those normals; an all-zero
    noise buffer = noisy = 0.  Actions equal, q within the act tolerance."""
    m = ctx.mem
    row = 1 if ctx.n_max > 1 else 0
    ctx.ad.reset_noise_online(ctx.raw_np[row])
    want_a, want_q = ctx.act_shared(n, 1)
    rep = m.upload(np.repeat(m.download(ctx.noise)[row:row + 1], n, axis=0))
    a, q = ctx.act_rows(n, noise=rep)
    assert np.array_equal(a, want_a) and close_q(q, want_q), q_error_share(q, want_q)
    want_a, want_q = ctx.act_shared(n, 0)
    a, q = ctx.act_rows(n, noise=m.upload(np.zeros((n, ctx.n_noise), dtype=np.float32)))
    assert np.array_equal(a, want_a) and close_q(q, want_q), q_error_share(q, want_q)


# =============================================================================== 3. locality
def check_locality(ctx, n, split):
    """Twice the same call: bit-identical.  [0, n) as [0, split) + [split, n): equal actions, q within tolerance (another
    m-tile shape may sum in another order).  One row's state and noise changed: every OTHER row keeps its action and q bits."""
    m = ctx.mem
    a1, q1 = ctx.act_rows(n)
    a2, q2 = ctx.act_rows(n)
    assert np.array_equal(a1, a2) and np.array_equal(bits(q1), bits(q2))
    st, nz = ctx.states_np[:n], m.download(ctx.noise)[:n]
    pa, pq = [], []
    for lo, hi in ((0, split), (split, n)):
        a, q = ctx.act_rows(hi - lo, states=m.upload(st[lo:hi]), noise=m.upload(nz[lo:hi]))
        pa.append(a)
        pq.append(q)
    assert np.array_equal(np.concatenate(pa), a1) and close_q(np.concatenate(pq), q1)
    victim = n // 2
    st2, nz2 = st.copy(), nz.copy()
    st2[victim] = st[(victim + 1) % n][::-1]
    nz2[victim] = nz[(victim + 1) % n]
    a3, q3 = ctx.act_rows(n, states=m.upload(st2), noise=m.upload(nz2))
    keep = np.arange(n) != victim
    assert np.array_equal(a3[keep], a1[keep]) and np.array_equal(bits(q3)[keep], bits(q1)[keep])
    assert bits(q3)[victim] != bits(q1)[victim]


# =============================================================================== 4. the generator
def check_generator(ctx):
    """Counter-based and stateless: replays, splits with row0, moves with round / row / the high half of a 64-bit seed; writes
    [rows][n_noise] and nothing else, uncovered floats zero."""
    m = ctx.mem
    seed, rnd = 0x1234, 7

    def learner_rng():
        s, e = C.c_uint64(0), C.c_uint64(0)
        L.check(ctx.lib, ctx.lib.rb_learner_get_rng(ctx.ad.h, C.byref(s), C.byref(e), m.stream))
        return s.value, e.value

    rng_before = learner_rng()
    whole = ctx.generate(33, 0, seed, rnd)
    assert learner_rng() == rng_before              # the learner's own (seed, epoch) is neither read nor advanced
    assert np.array_equal(bits(whole), bits(ctx.generate(33, 0, seed, rnd)))
    parts = np.concatenate([ctx.generate(16, 0, seed, rnd), ctx.generate(17, 16, seed, rnd)])
    assert np.array_equal(bits(whole), bits(parts))
    live = ctx.live_mask()
    assert live.sum() == ctx.draws and live.sum() < ctx.n_noise, "this shape's noise layout has no padding to check"
    assert not whole[:, ~live].any()
    assert np.isfinite(whole).all() and (np.abs(whole[:, live]) > 0).mean() > 0.99
    rows = whole[:, live]
    assert len({r.tobytes() for r in rows}) == 33                                     # other rows, other values
    assert not np.array_equal(ctx.generate(2, 0, seed, rnd + 1)[:, live], rows[:2])     # other rounds
    assert not np.array_equal(ctx.generate(2, 0, seed, rnd + (1 << 32))[:, live], rows[:2])
    for other in (seed + (1 << 32), seed + (1 << 63)):                                # seeds that differ only above bit 32
        got = ctx.generate(2, 0, other, rnd)[:, live]
        assert not np.array_equal(got[0], rows[0]) and not np.array_equal(got[1], rows[1])
    # sentinels around the destination inside a larger allocation, rows = 17
    pad, R = 64, 17
    big = m.upload(np.full(pad + R * ctx.n_noise + pad, -777.0, dtype=np.float32))
    ctx.fill(big, R, 16, seed, rnd, offset=pad)
    got = m.download(big)
    assert (got[:pad] == -777.0).all() and (got[-pad:] == -777.0).all()
    assert np.array_equal(bits(got[pad:-pad].reshape(R, ctx.n_noise)), bits(whole[16:33]))


def check_injected_normals(ctx):
    """Injected normals: row i is make_noise of ITS block, to the bits (f(x) = sign(x) sqrt|x| is one correctly rounded square
    root on either build and in numpy: no ulp of slack), zero elsewhere."""
    got = ctx.mem.download(ctx.noise)
    from cabi_adapter import query_layout
    layout = query_layout(ctx.lib, ctx.ad.cfg, ctx.lib.rb_learner_noise_layout)
    for i in range(ctx.n_max):
        want = np.zeros(ctx.n_noise, dtype=np.float32)
        for layer, (e_in, e_out) in O.make_noise(ctx.cfg, ctx.raw_np[i]).items():
            for part, v in (("eps_in", e_in), ("eps_out", e_out)):
                off, shp = layout["%s.%s" % (layer, part)]
                assert shp == v.shape
                want[off:off + v.size] = v
        assert np.array_equal(bits(got[i]), bits(want)), i


def check_generator_statistics(ctx, rows=128):
    """rows x draws > 10^6 values of the device generator: the moment, KS and lag-1 bounds of test_device_rng_noise_statistics
    (formulas in n), and the correlation between two rows below 5 / sqrt(len)."""
    import math
    from scipy import stats
    live = ctx.live_mask()
    x = ctx.generate(rows, 0, 99, 3)[:, live].astype(np.float64)
    a, b = x[0], x[rows // 2]
    x = x.ravel()
    assert x.size >= 1_000_000
    g = np.sign(x) * x * x                            # invert f: g ~ N(0,1) if and only if x ~ f(N(0,1))
    n = g.size
    assert abs(g.mean()) < 5.0 / math.sqrt(n)
    assert abs(g.var() - 1.0) < 5.0 * math.sqrt(2.0 / n)
    assert abs((g ** 4).mean() - 3.0) < 5.0 * math.sqrt(96.0 / n)
    assert abs((g ** 3).mean()) < 5.0 * math.sqrt(15.0 / n)
    d, _p = stats.kstest(g, "norm")
    assert d < 1.95 / math.sqrt(n), d
    want = 2 ** 0.25 * math.gamma(0.75) / math.sqrt(math.pi)
    assert abs(np.abs(x).mean() - want) < 5.0 * math.sqrt((math.sqrt(2 / math.pi) - want ** 2) / n)
    assert abs(np.corrcoef(g[:-1], g[1:])[0, 1]) < 5.0 / math.sqrt(n)
    assert abs(np.corrcoef(a, b)[0, 1]) < 5.0 / math.sqrt(a.size)


# =============================================================================== 5. refusals
def check_refusals(ctx):
    lib, m, h = ctx.lib, ctx.mem, ctx.ad.h
    st = m.upload(ctx.states_np[:2])
    a, q = m.upload(np.full(2, -5, dtype=np.int32)), m.upload(np.full(2, -5.0, dtype=np.float32))
    nz = m.upload(np.full((2, ctx.n_noise), -9.0, dtype=np.float32))

    def refused(fn, name, word, *args):
        assert fn(*args) == -1
        msg = lib.rb_last_error()
        assert name in msg and word in msg, msg

    act, gen = lib.rb_learner_act_batch_rows, lib.rb_learner_noise_rows
    refused(act, b"rb_learner_act_batch_rows", b"NULL handle", None, m.ptr(st), 2, m.ptr(nz), m.ptr(a), m.ptr(q), m.stream)
    refused(act, b"rb_learner_act_batch_rows", b"states_dev", h, None, 2, m.ptr(nz), m.ptr(a), m.ptr(q), m.stream)
    refused(act, b"rb_learner_act_batch_rows", b"noise_rows_dev", h, m.ptr(st), 2, None, m.ptr(a), m.ptr(q), m.stream)
    for n in (0, 257, -1):
        refused(act, b"rb_learner_act_batch_rows", b"n must be", h, m.ptr(st), n, m.ptr(nz), m.ptr(a), m.ptr(q), m.stream)
    refused(gen, b"rb_learner_noise_rows", b"NULL handle", None, 2, 0, 1, 1, None, m.ptr(nz), m.stream)
    refused(gen, b"rb_learner_noise_rows", b"noise_rows_dev", h, 2, 0, 1, 1, None, None, m.stream)
    for rows in (0, 257, -1):
        refused(gen, b"rb_learner_noise_rows", b"rows must be", h, rows, 0, 1, 1, None, m.ptr(nz), m.stream)
    refused(gen, b"rb_learner_noise_rows", b"row0", h, 2, -1, 1, 1, None, m.ptr(nz), m.stream)
    m.sync()
    assert m.download(a).tolist() == [-5, -5] and m.download(q).tolist() == [-5.0, -5.0]      # nothing ran
    assert (m.download(nz) == -9.0).all()
