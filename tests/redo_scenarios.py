"""Recycling dormant units (rb_learner_unit_activity / _dormant_mask / _recycle_units, csrc/unit_recycle.h) against
tests/redo_oracle.py.  Shared by tests/test_redo_emu.py (NumpyMem, host interpreter) and tests/test_redo_gpu.py (TorchMem).

The nets are those of tests/reset_scenarios.py at batch 4, history 4 — the smallest that still cross every branch:
  de64      data-efficient, hidden 64, atoms 51, actions 3: the last conv has P = 9 (F-columns in runs of 9), fc_z_a sits 51 floats
            into its segment
  de48      hidden 48, atoms 2, actions 1: hidden is no multiple of the wave; the outgoing columns of a hidden unit are 2 elements
  canon48   canonical, hidden 48, atoms 21, actions 4: three conv layers, the conv -> conv outgoing slices (ks^2 = 16 and 9), P = 49
  de48-h1   history 1: the first layer's rows are K = 25 floats, so they start and end inside quads
  canon48-h1  history 1: K = 64 (the recycle body only: no forward is involved in what changes)

Tolerances.  activity: |activity - sum_f64| <= count 2^-53 sum |h| per unit (the issue's bound: any order of `count` float64
additions of float32 terms stays inside it).  Activations against oracle/learner_oracle.py's eval-mode forward: rtol 2e-5, atol 1e-6,
the tolerance of the project's forward tests at these shapes (head_shapes_scenarios.ACT_RTOL / ACT_ATOL, test_learner_gpu's
evaluate_q checks).  Mask, counts and every recycled bit: exact.  Scores: 1 float32 ulp of the float64 quotient."""
import ctypes as C

import numpy as np

import diag_scenarios as DS
import optimizer_scenarios as S
import redo_oracle as RD
import reset_scenarios as R
import scenarios
from cabi_adapter import CAbiLearnAdapter, learner_config, query_layout
from head_shapes_scenarios import ACT_ATOL, ACT_RTOL
from helpers import assert_learn_trace_matches
from learn_steps import RELU_MARGIN, OracleRun, conv_shapes, two_step_inputs
from oracle import learner_oracle as O
from rainbow_amd import _lib as L

F32 = np.float32
RB_ERR_INVALID, RB_ERR_STATE = -1, -4
ROWS = {"de64": ("de64", 4), "de48": ("de48", 4), "canon48": ("canon48", 4), "de48-h1": ("de48", 1)}
RECYCLE_ROWS = dict(ROWS, **{"canon48-h1": ("canon48", 1)})
STD, SEED, DRAW = R.STD, R.SEED, R.DRAW
TAUS = (0.0, 0.1, 0.5, 1.0, 4.0)
_bits, _store, same = R._bits, R._store, R.same


def row_config(row):
    net, hist = RECYCLE_ROWS[row]
    return dict(R.NETS[net], batch=4, multi_step=3, discount=0.99, history=hist, v_min=-10.0, v_max=10.0)


class Rig(R.Rig):
    """reset_scenarios.Rig for a row of this file (its history), with the unit layout and the three entry points."""

    def __init__(self, lib, Mem, row, learner_seed=1234):
        self.lib, self.mem = lib, Mem()
        m = self.mem
        self.c = row_config(row)
        self.cfg = learner_config(self.c)
        n_params, n_noise = C.c_int64(0), C.c_int64(0)
        L.check(lib, lib.rb_learner_sizes(C.byref(self.cfg), C.byref(n_params), C.byref(n_noise)))
        self.n = n_params.value
        self.layout = query_layout(lib, self.cfg, lib.rb_learner_param_layout)
        self.bufs = {k: m.empty((self.n,), np.float32) for k in "ptgmv"}
        self.noise = [m.empty((n_noise.value,), np.float32) for _ in range(2)]
        self.h = C.c_void_p()
        b = self.bufs
        L.check(lib, lib.rb_learner_create(C.byref(self.h), C.byref(self.cfg), m.ptr(b["p"]), m.ptr(b["t"]), m.ptr(b["g"]),
                                           m.ptr(self.noise[0]), m.ptr(self.noise[1]), learner_seed))
        self.units = unit_layout(lib, self.cfg)
        self.U = int(sum(self.units))

    def flat(self, params):
        out = np.zeros(self.n, F32)
        for name, (off, shape) in self.layout.items():
            out[off:off + int(np.prod(shape))] = np.asarray(params[name], dtype=F32).ravel()
        return out

    def unflat(self, flat):
        return {name: flat[off:off + int(np.prod(shape))].reshape(shape).copy() for name, (off, shape) in self.layout.items()}

    def debug(self, what, shape):
        out = self.mem.empty(shape, np.float32)
        L.check(self.lib, self.lib.rb_learner_debug_read(self.h, what, self.mem.ptr(out), self.mem.stream))
        self.mem.sync()
        return self.mem.download(out)

    def activations(self):
        """(conv activations per layer, hidden activations) of the last forward, rows [0, B)."""
        B = self.c["batch"]
        cfg = O.Config(**self.c)
        return [self.debug(6 + i, shp) for i, shp in enumerate(conv_shapes(cfg, B))], self.debug(5, (B, 2 * self.c["hidden"]))

    def activity(self, states_buf, accumulate, act_buf):
        return self.lib.rb_learner_unit_activity(self.h, self.mem.ptr(states_buf), accumulate, self.mem.ptr(act_buf), self.mem.stream)

    def mask(self, act_buf, tau, mask_buf, counts_buf, scores_buf=None):
        m = self.mem
        return self.lib.rb_learner_dormant_mask(self.h, m.ptr(act_buf), tau, m.ptr(mask_buf), m.ptr(counts_buf),
                                                m.ptr(scores_buf) if scores_buf is not None else None, m.stream)

    def recycle(self, mask, seed=SEED, draw=DRAW, with_target=1, moments=True, std=STD):
        m, b = self.mem, self.bufs
        self._mask = m.upload(np.asarray(mask, dtype=np.uint8))        # (kept alive until the stream has consumed it)
        return self.lib.rb_learner_recycle_units(self.h, m.ptr(self._mask), std, seed, draw, with_target,
                                                 m.ptr(b["m"]) if moments else None, m.ptr(b["v"]) if moments else None, m.stream)


def unit_layout(lib, cfg):
    n, units = C.c_int32(0), (C.c_int32 * 5)()
    L.check(lib, lib.rb_learner_unit_layout(C.byref(cfg), C.byref(n), units))
    assert all(u == 0 for u in units[n.value:])
    return [int(u) for u in units[:n.value]]


def layout_check(lib, Mem, row):
    """rb_learner_unit_layout against the oracle's reading of rb_learner_param_layout."""
    rig = Rig(lib, Mem, row)
    want = RD.unit_layout(rig.layout)
    assert rig.units == [n for _, n in want], (rig.units, want)
    nconv = 3 if rig.c["architecture"] == "canonical" else 2
    assert len(rig.units) == nconv + 2 and rig.units[-2:] == [rig.c["hidden"]] * 2
    n = C.c_int32(0)
    L.check(lib, lib.rb_learner_unit_layout(C.byref(rig.cfg), C.byref(n), None))
    assert n.value == nconv + 2
    assert lib.rb_learner_unit_layout(C.byref(rig.cfg), None, None) == RB_ERR_INVALID
    rig.close()


# =============================================================================== 1: activity
def oracle_activations(c, params, states_u8):
    """The eval-mode forward of oracle/learner_oracle.py: (post-ReLU conv activations per layer, hidden activations [B, 2H]).  The
    oracle reports its conv pre-activations only when it is handed the ReLU decisions, so it is handed its OWN, layer by layer."""
    import torch
    cfg = O.Config(**c)
    p = {k: torch.as_tensor(np.ascontiguousarray(v)) for k, v in params.items()}
    x = torch.as_tensor(states_u8).to(torch.float32).div(255)
    shapes = conv_shapes(cfg, c["batch"])
    masks = [np.ones(s, bool) for s in shapes]
    with torch.no_grad():
        for i in range(len(shapes) + 1):
            probe = {}
            O.forward(cfg, p, None, x, probe=probe, conv_masks=masks)
            if i < len(shapes):
                masks[i] = probe["conv_pre"][i] > 0
    return [np.maximum(pre, 0).astype(F32) for pre in probe["conv_pre"]], np.maximum(probe["hidden_pre"], 0).astype(F32)


def random_states(c, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(c["batch"], c["history"], 84, 84)).astype(np.uint8)


def load_net(rig, seed, same_target=False):
    cfg = O.Config(**rig.c)
    online = O.init_params(cfg, seed)
    target = online if same_target else O.init_params(cfg, seed + 1000)
    st = dict(p=rig.flat(online), t=rig.flat(target), m=np.zeros(rig.n, F32), v=np.zeros(rig.n, F32), g=np.zeros(rig.n, F32))
    rig.load(st)
    return online, st


def assert_activity(what, act, conv_acts, h, scale=1.0):
    s, a, n = RD.per_unit(conv_acts, h)
    err, bound = np.abs(np.asarray(act, dtype=np.float64) - scale * s), n * 2.0 ** -53 * a
    pos = bound > 0
    print("redo activity %s: largest error / bound %.3g (%d units, %d of them all-zero)"
          % (what, float((err[pos] / bound[pos]).max()) if pos.any() else 0.0, act.size, int((~pos).sum())))
    assert np.all(err <= bound), (what, int(np.argmax(err - bound)), float(err.max()))
    return s


def activity_check(lib, Mem, row):
    """rb_learner_unit_activity on random u8 states: every unit's sum against the float64 sum of the activations read back
    (selectors 5 - 8); accumulate = 1 gives the doubled sum within the same bound; a repeated run is bit-identical; the activations
    match the oracle's eval-mode forward although both noise buffers hold non-zero draws; no caller buffer changes."""
    rig = Rig(lib, Mem, row)
    m = rig.mem
    online, _ = load_net(rig, 5)
    rs = np.random.RandomState(3)
    for nb in rig.noise:
        _store(nb, rs.randn(nb.shape[0]).astype(F32))
    m.sync()
    before, noise_before = rig.state(), [m.download(nb).copy() for nb in rig.noise]
    states = random_states(rig.c, 17)
    sbuf = m.upload(states)
    act = m.upload(np.full(rig.U, 7.0, np.float64))                       # (accumulate = 0 overwrites whatever is there)
    L.check(lib, rig.activity(sbuf, 0, act))
    m.sync()
    a1 = m.download(act).copy()
    conv_acts, h = rig.activations()
    assert_activity(row, a1, conv_acts, h)
    L.check(lib, rig.activity(sbuf, 1, act))
    m.sync()
    a2 = m.download(act).copy()
    assert_activity(row + " accumulated", a2, conv_acts, h, scale=2.0)
    act3 = m.empty((rig.U,), np.float64)
    L.check(lib, rig.activity(sbuf, 0, act3))
    m.sync()
    assert np.array_equal(m.download(act3).view(np.uint64), a1.view(np.uint64)), "a repeated run must be bit-identical"
    want_conv, want_h = oracle_activations(rig.c, online, states)
    for i, (got, want) in enumerate(zip(conv_acts + [h], want_conv + [want_h])):
        np.testing.assert_allclose(got, want, rtol=ACT_RTOL, atol=ACT_ATOL, err_msg="%s: activations of layer %d" % (row, i))
    same(rig.state(), before, (row, "rb_learner_unit_activity must not write a caller's buffer"))
    for nb, nb0 in zip(rig.noise, noise_before):
        assert np.array_equal(_bits(m.download(nb)), _bits(nb0)), "the noise buffers must stay as they are"
    for i, arg in ((1, "states_dev"), (3, "activity_dev")):
        a = [rig.h, m.ptr(sbuf), 0, m.ptr(act), m.stream]
        a[i] = None
        assert lib.rb_learner_unit_activity(*a) == RB_ERR_INVALID and arg.encode() in lib.rb_last_error(), arg
    rig.close()


def _measure(lib, mem, ad, states_buf, bufs, tau=0.1):
    L.check(lib, lib.rb_learner_unit_activity(ad.h, mem.ptr(states_buf), 0, mem.ptr(bufs["act"]), mem.stream))
    L.check(lib, lib.rb_learner_dormant_mask(ad.h, mem.ptr(bufs["act"]), tau, mem.ptr(bufs["mask"]), mem.ptr(bufs["counts"]),
                                             mem.ptr(bufs["scores"]), mem.stream))
    mem.sync()


def _measure_bufs(lib, mem, ad):
    units = unit_layout(lib, ad.cfg)
    U = int(sum(units))
    return dict(act=mem.empty((U,), np.float64), mask=mem.empty((U,), np.uint8), counts=mem.empty((len(units),), np.int32),
                scores=mem.empty((U,), np.float32))


def no_side_effects_check(lib, mem):
    """diag_scenarios.check_eval_no_side_effects with the activity and mask launches in place of the held-out loss: twins run
    train_step (the pass left pending); one of them measures in between.  Around the measurement (after rb_learner_flush) parameters,
    target, moments, gradients, both noise buffers, the noise epoch, the step counter, the norm and the sink's tree are bit-identical,
    and the next step equals the twin's."""
    c = DS.case_config("z51-a6")
    hs = [DS.ts_build(lib, mem, c, "_redo_se%d" % i, flags=L.LEARNER_DEFER_UPDATE) for i in range(2)]
    try:
        def rng(ad):
            s, e = C.c_uint64(0), C.c_uint64(0)
            L.check(lib, lib.rb_learner_get_rng(ad.h, C.byref(s), C.byref(e), mem.stream))
            return s.value, e.value
        for rp, ad, o, job in hs:
            DS.ts_call(lib, mem, c, rp, ad, o, job)
        rp, ad, o, job = hs[0]
        L.check(lib, lib.rb_learner_flush(ad.h, mem.stream))
        before, rng_before = DS.ts_state(mem, rp, ad, o), rng(ad)
        sbuf = mem.upload(random_states(c, 99))
        bufs = _measure_bufs(lib, mem, ad)
        _measure(lib, mem, ad, sbuf, bufs)
        after, rng_after = DS.ts_state(mem, rp, ad, o), rng(ad)
        assert rng_before == rng_after
        for k in before:
            assert DS.same_bits(before[k], after[k]), "rb_learner_unit_activity / rb_learner_dormant_mask changed %s" % k
        assert np.isfinite(mem.download(bufs["act"])).all() and float(mem.download(bufs["act"]).sum()) > 0
        # a pending pass runs first: twin 0 measures with its pass pending, twin 1 never measures
        for rp, ad, o, job in hs:
            DS.ts_call(lib, mem, c, rp, ad, o, job)
        _measure(lib, mem, hs[0][1], sbuf, bufs)
        for rp, ad, o, job in hs:
            DS.ts_call(lib, mem, c, rp, ad, o, job)
        for rp, ad, o, job in hs:
            L.check(lib, lib.rb_learner_flush(ad.h, mem.stream))
        a, b = DS.ts_state(mem, *hs[0][:3]), DS.ts_state(mem, *hs[1][:3])
        for k in a:
            assert DS.same_bits(a[k], b[k]), "the steps after the measurement differ from the twin's in %s" % k
        assert rng(hs[0][1]) == rng(hs[1][1])
    finally:
        for i, (rp, ad, o, job) in enumerate(hs):
            ad.close(); rp.close()
            DS.drop_config("_redo_se%d" % i)


def refusal_check(lib, mem):
    """While the gradients of a learn call wait for rb_learner_finish_grads (replica exchange armed, the setup of
    diag_scenarios.check_exchange_gives_nan) the activity call refuses, and works again afterwards."""
    import exchange_scenarios as XS
    c = DS.case_config("z51-a6")
    _cfg, online, target, steps = DS.learn_inputs(c, 11, steps=1)
    ad, name = DS.make_learner(lib, mem, "redo-xch", c)
    try:
        ad.load(online, target)
        stride = XS.exchange_layout(lib, ad)[0]
        lo, al = mem.upload(np.zeros(stride, dtype=np.float32)), mem.empty((2 * stride,), np.float32)
        L.check(lib, lib.rb_learner_set_exchange(ad.h, 2, mem.ptr(lo), mem.ptr(al)))
        st = steps[0]
        ad.reset_noise_online(st["raw_on"])
        ad.learn_only(st["batch"], st["raw_tg"])
        sbuf = mem.upload(random_states(c, 5))
        bufs = _measure_bufs(lib, mem, ad)
        args = (ad.h, mem.ptr(sbuf), 0, mem.ptr(bufs["act"]), mem.stream)
        assert lib.rb_learner_unit_activity(*args) == RB_ERR_STATE
        assert b"rb_learner_finish_grads" in lib.rb_last_error()
        XS.fill(al, np.concatenate([mem.download(lo), mem.download(lo)]))
        L.check(lib, lib.rb_learner_finish_grads(ad.h, mem.stream))
        L.check(lib, lib.rb_learner_unit_activity(*args))
        mem.sync()
        assert np.isfinite(mem.download(bufs["act"])).all()
    finally:
        lib.rb_learner_set_exchange(ad.h, 1, None, None)
        ad.close()
        DS.drop_config(name)


# =============================================================================== 2: mask
def planted_activities(units, variant):
    """Whole numbers (any summation order is exact).  Variant 0, layer by layer: [0] one unit holds 1 and the others add up to 2 N - 1, so
    that S = 2 N and, at tau = 0.5, activity * N == tau * S holds exactly for it (dormant); [1] all zero (dormant as a whole, at
    every tau); [2] a single NaN among small numbers (nothing dormant); [3] one live unit; [4] (canonical) small random numbers with
    zeros.  Variant 1 rotates the layers by one."""
    rs = np.random.RandomState(7 + variant)
    out = []
    for k, n in enumerate(units):
        kind = (k + variant) % len(units)
        a = np.zeros(n, np.float64)
        if kind == 0:
            a[:] = rs.multinomial(2 * n - 1, np.ones(n - 1) / (n - 1))[np.r_[0, 0:n - 1]]
            a[0] = 1.0                                          # S = 2 N: a[0] * N == 0.5 * S
        elif kind == 2:
            a[:] = rs.randint(0, 5, size=n)
            a[n // 3] = np.nan
        elif kind == 3:
            a[n - 1] = 6.0
        elif kind == 4:
            a[:] = rs.randint(0, 4, size=n) * rs.randint(0, 2, size=n)
        out.append(a)
    return np.concatenate(out)


def mask_check(lib, Mem, row):
    """Planted whole-number activities: mask and counts equal the oracle exactly at every tau of TAUS, scores within one float32 ulp of
    the float64 quotient; the planted cases are asserted to be there.  tau < 0, NaN and inf are refused and write nothing."""
    rig = Rig(lib, Mem, row)
    m = rig.mem
    f = RD.firsts(rig.layout)
    for variant in (0, 1):
        act = planted_activities(rig.units, variant)
        abuf = m.upload(act)
        seen_equal = seen_zero_layer = seen_nan = seen_live = False
        for tau in TAUS:
            mask, counts, scores = m.upload(np.full(rig.U, 9, np.uint8)), m.upload(np.full(len(rig.units), -1, np.int32)), \
                m.upload(np.full(rig.U, -1.0, F32))
            L.check(lib, rig.mask(abuf, tau, mask, counts, scores))
            m.sync()
            want_mask, want_counts, want_scores = RD.dormant(rig.layout, act, tau)
            got_mask, got_counts, got_scores = m.download(mask), m.download(counts), m.download(scores)
            assert np.array_equal(got_mask, want_mask), (row, variant, tau, np.flatnonzero(got_mask != want_mask)[:8])
            assert np.array_equal(got_counts, want_counts), (row, variant, tau, got_counts, want_counts)
            w32 = want_scores.astype(F32)
            fin = np.isfinite(w32)
            assert np.array_equal(np.isnan(got_scores), np.isnan(w32))
            assert np.all(np.abs(got_scores[fin].astype(np.float64) - w32[fin]) <= np.spacing(np.abs(w32[fin]))), (row, variant, tau)
            for k in range(len(rig.units)):
                a, d = act[f[k]:f[k + 1]], want_mask[f[k]:f[k + 1]]
                S = a.sum()
                seen_equal |= bool(np.any((a * a.size == tau * S) & (a > 0)) and d[np.flatnonzero((a * a.size == tau * S) & (a > 0))].all())
                seen_zero_layer |= bool(not a.any() and d.all())
                seen_nan |= bool(np.isnan(a).any() and not d.any())
                seen_live |= bool((a > 0).sum() == 1 and d.sum() == a.size - 1)
            L.check(lib, rig.mask(abuf, tau, mask, counts, None))                   # scores are optional
            m.sync()
            assert np.array_equal(m.download(mask), want_mask)
        assert seen_equal and seen_zero_layer and seen_nan and seen_live, (seen_equal, seen_zero_layer, seen_nan, seen_live)
    mask, counts = m.upload(np.full(rig.U, 9, np.uint8)), m.upload(np.full(len(rig.units), -1, np.int32))
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert rig.mask(abuf, bad, mask, counts) == RB_ERR_INVALID and b"tau" in lib.rb_last_error(), bad
    m.sync()
    assert np.all(m.download(mask) == 9) and np.all(m.download(counts) == -1), "a refused call must write nothing"
    rig.close()


# =============================================================================== 3: recycle, bit for bit
def masks_of(rig):
    f = RD.firsts(rig.layout)
    U = rig.U
    one = np.zeros(U, np.uint8)
    for k, n in enumerate(rig.units):
        one[f[k] + (3 * k + 2) % n] = 1
    ends = np.zeros(U, np.uint8)
    ends[f[:-1]] = 1
    ends[f[1:] - 1] = 1
    pair = np.zeros(U, np.uint8)                   # two adjacent layers that meet in one element: the last two conv layers and fc_h_a
    nconv = len(rig.units) - 2
    pair[f[nconv - 2] + 5] = pair[f[nconv - 1] + 7] = pair[f[nconv + 1] + 11] = 1
    return {"empty": np.zeros(U, np.uint8), "one-per-layer": one, "first-and-last": ends, "adjacent": pair, "every": np.ones(U, np.uint8)}


def recycle_check(lib, Mem, row):
    """Parameters, target and both moments equal the oracle in every bit for the five masks; every untouched element is byte-identical
    to before; the gradient is never touched; the empty mask changes nothing; with_target = 0 and NULL moments leave those buffers
    alone; phi of an element is the same whether its unit is recycled alone or with all the others."""
    rig = Rig(lib, Mem, row)
    masks = masks_of(rig)
    got_by = {}
    runs = [(name, 1, True) for name in masks] + [("first-and-last", 0, True), ("first-and-last", 1, False), ("adjacent", 0, False)]
    for k, (name, wt, mom) in enumerate(runs):
        st = rig.fill(70 + k)
        L.check(lib, rig.recycle(masks[name], with_target=wt, moments=mom))
        got = rig.state()
        want, kind, both = RD.recycle(rig.layout, st, masks[name], STD, SEED, DRAW, with_target=bool(wt), moments=mom)
        want["g"] = st["g"]
        same(got, want, (row, name, wt, mom))
        untouched = kind == RD.UNTOUCHED
        for key in "ptmv":
            assert np.array_equal(_bits(got[key][untouched]), _bits(st[key][untouched])), (row, name, key, "an untouched element changed")
        if name == "empty":
            same(got, st, (row, "the empty mask must change nothing"))
        else:
            assert (~untouched).any() and not np.array_equal(_bits(got["p"][~untouched]), _bits(st["p"][~untouched]))
        if name in ("adjacent", "one-per-layer", "every"):
            assert both > 0, (row, name, "the mask must make two dormant units meet in one element")
        if not wt:
            assert np.array_equal(_bits(got["t"]), _bits(st["t"]))
        if not mom:
            assert np.array_equal(_bits(got["m"]), _bits(st["m"])) and np.array_equal(_bits(got["v"]), _bits(st["v"]))
        if (wt, mom) == (1, True):
            got_by[name] = (got["p"], kind)
    (p_one, k_one), (p_all, k_all) = got_by["one-per-layer"], got_by["every"]
    shared = (k_one == RD.INCOMING) & (k_all == RD.INCOMING)
    assert shared.sum() >= 20 and np.array_equal(_bits(p_one[shared]), _bits(p_all[shared])), "phi must not depend on the other units"
    # the layout's padding and the output layer's biases belong to no unit
    covered = np.zeros(rig.n, bool)
    for name, (off, shape) in rig.layout.items():
        if not (name.startswith("fc_z") and ".bias" in name):
            covered[off:off + int(np.prod(shape))] = True
    assert not (k_all != RD.UNTOUCHED)[~covered].any() and (k_all != RD.UNTOUCHED)[covered].all()
    rig.close()


def bad_inputs_check(lib, Mem, row):
    """phi and the outgoing values are written without reading theta: NaN and inf planted in the recycled elements of the online and
    the target parameters do not survive; everything else keeps its (non-finite) bits."""
    rig = Rig(lib, Mem, row)
    mask = masks_of(rig)["first-and-last"]
    st = rig.fill(31)
    _want, kind, _both = RD.recycle(rig.layout, st, mask, STD, SEED, DRAW)
    rs = np.random.RandomState(5)
    touched = kind != RD.UNTOUCHED
    for k, bad in (("p", np.nan), ("t", np.inf)):
        plant = touched & (rs.rand(rig.n) < 0.25)
        plant[np.flatnonzero(touched)[[0, -1]]] = True
        st[k][plant] = bad
        st[k][plant & (rs.rand(rig.n) < 0.5)] = -np.inf if k == "p" else np.nan
        st[k][np.flatnonzero(~touched)[::97]] = bad                          # ... and outside: those must stay
    rig.load(st)
    L.check(lib, rig.recycle(mask))
    got = rig.state()
    want, _kind, _both = RD.recycle(rig.layout, st, mask, STD, SEED, DRAW)
    same(got, want, (row, "non-finite inputs"), keys="ptmv")
    assert np.isfinite(got["p"][touched]).all() and np.isfinite(got["t"][touched]).all()
    assert np.array_equal(_bits(got["p"][touched]), _bits(got["t"][touched]))
    rig.close()


def keys_check(lib, Mem, row):
    """Another draw and another seed give another phi; the learner's own seed does not enter; refused arguments change nothing."""
    a, b = Rig(lib, Mem, row, learner_seed=1), Rig(lib, Mem, row, learner_seed=99)
    mask = masks_of(a)["every"]
    ps = {}
    for tag, rig, seed, draw in (("a0", a, 7, 0), ("a1", a, 7, 1), ("b0", b, 7, 0), ("s8", b, 8, 0)):
        st = rig.fill(3)
        L.check(lib, rig.recycle(mask, seed=seed, draw=draw))
        ps[tag] = rig.state()["p"]
        want, kind, _ = RD.recycle(rig.layout, st, mask, STD, seed, draw)
        assert np.array_equal(_bits(ps[tag]), _bits(want["p"])), tag
    drawn = (kind == RD.INCOMING) & (RD.phi_flat(a.layout, a.n, STD, 7, 0) != RD.phi_flat(a.layout, a.n, STD, 7, 1))
    assert np.array_equal(_bits(ps["a0"]), _bits(ps["b0"])), "the learner's own seed must not enter the draw"
    for other in ("a1", "s8"):
        assert float(np.mean(ps["a0"][drawn] != ps[other][drawn])) > 0.99, other
    st = a.fill(4)
    m = a.mem
    assert a.recycle(mask, std=float("nan")) == RB_ERR_INVALID and b"noisy_std" in lib.rb_last_error()
    assert lib.rb_learner_recycle_units(a.h, m.ptr(a._mask), STD, 1, 1, 1, m.ptr(a.bufs["m"]), None, m.stream) == RB_ERR_INVALID
    assert lib.rb_learner_recycle_units(a.h, None, STD, 1, 1, 1, None, None, m.stream) == RB_ERR_INVALID and b"mask_dev" in lib.rb_last_error()
    same(a.state(), st, "a refused call must change nothing")
    a.close(); b.close()


# =============================================================================== 4: function preserved, unit revived
def kill_units(rig, params, killed):
    """Incoming weights 0 (sigma parts too), bias -1: the unit's pre-activation is exactly -1 on every input.  Every other unit gets
    the absolute values of its initial incoming weights (conv weights and fc_h weight_mu): on noise images a channel's
    pre-activations nearly all share one sign, and a fifth of the channels of a fresh net are silent on their own; with non-negative
    weights on non-negative inputs every unit fires.  The caller asserts from the oracle alone that every unit that was not killed
    is alive on its batch."""
    p = {k: np.array(v, copy=True) for k, v in params.items()}
    for name in RD.conv_names(rig.layout) + [s + ".weight_mu" for s in RD.HIDDEN]:
        p[name] = np.abs(p[name])
    flat = rig.flat(p)
    for u in killed:
        inc, _o0, _oc = RD.index_sets(rig.layout, u)
        flat[inc] = 0.0
    for u in killed:
        inc, _o0, _oc = RD.index_sets(rig.layout, u)
        f = RD.firsts(rig.layout)
        k = int(np.searchsorted(f, u, side="right")) - 1
        names = RD.conv_names(rig.layout)
        bias = (rig.layout[names[k].replace("weight", "bias")][0] if k < len(names) else rig.layout[RD.HIDDEN[k - len(names)] + ".bias_mu"][0])
        flat[bias + int(u - f[k])] = -1.0
    return flat


def eval_loss(rig, batch_bufs, loss_buf):
    m = rig.mem
    L.check(rig.lib, rig.lib.rb_learner_eval_loss(rig.h, m.ptr(batch_bufs["states"]), m.ptr(batch_bufs["next_states"]),
                                                   m.ptr(batch_bufs["actions"]), m.ptr(batch_bufs["returns"]),
                                                   m.ptr(batch_bufs["nonterminals"]), m.ptr(loss_buf), None, m.stream))
    m.sync()
    return m.download(loss_buf).copy()


def function_preserved_check(lib, Mem, row):
    """Killed units -> measure -> mask (tau = 0) -> recycle (target too): exactly the killed units are masked, the eval-mode per-sample
    loss on the same batch is numerically equal before and after, and a second measurement matches the oracle's forward on the
    recycled parameters."""
    rig = Rig(lib, Mem, row)
    m = rig.mem
    cfg = O.Config(**rig.c)
    f = RD.firsts(rig.layout)
    killed = sorted({int(f[k] + j % n) for k, n in enumerate(rig.units) for j in (1, 6, n - 1)})
    flat = kill_units(rig, O.init_params(cfg, 9), killed)
    rig.load(dict(p=flat, t=flat, m=np.zeros(rig.n, F32), v=np.zeros(rig.n, F32), g=np.zeros(rig.n, F32)))     # target = online
    batch = scenarios.make_batch(rig.c, 41)
    bufs = DS.upload_batch(m, rig.c, batch)
    # the oracle alone: the killed units, and no others, are silent on this batch; every other score is away from 0
    conv0, h0 = oracle_activations(rig.c, rig.unflat(flat), batch["states"])
    s0, _a, _n = RD.per_unit(conv0, h0)
    want_mask, _c, scores0 = RD.dormant(rig.layout, s0, 0.0)
    assert np.array_equal(np.flatnonzero(want_mask), killed), "ill-conditioned parameters: a unit is silent that was not killed"
    assert np.all(scores0[want_mask == 0] > 1e-6), "ill-conditioned parameters: a live unit's score lies at the threshold"
    loss = m.empty((rig.c["batch"],), np.float32)
    loss_before = eval_loss(rig, bufs, loss)
    act, mask, counts = m.empty((rig.U,), np.float64), m.empty((rig.U,), np.uint8), m.empty((len(rig.units),), np.int32)
    L.check(lib, rig.activity(bufs["states"], 0, act))
    L.check(lib, rig.mask(act, 0.0, mask, counts))
    L.check(lib, lib.rb_learner_recycle_units(rig.h, m.ptr(mask), STD, SEED, DRAW, 1, m.ptr(rig.bufs["m"]), m.ptr(rig.bufs["v"]), m.stream))
    m.sync()
    got_mask = m.download(mask)
    assert np.array_equal(np.flatnonzero(got_mask), killed), (row, np.flatnonzero(got_mask), killed)
    assert np.all(m.download(act)[got_mask == 1] == 0.0)
    assert int(m.download(counts).sum()) == len(killed)
    after = rig.state()
    want, kind, _both = RD.recycle(rig.layout, dict(p=flat, t=flat, m=np.zeros(rig.n, F32), v=np.zeros(rig.n, F32)), got_mask, STD, SEED, DRAW)
    same(after, want, (row, "the recycle behind the device's own mask"), keys="ptmv")
    loss_after = eval_loss(rig, bufs, loss)
    assert np.all(np.isfinite(loss_before)) and np.all(loss_before == loss_after), (row, loss_before, loss_after)
    # the second measurement: the oracle's forward on the recycled parameters
    L.check(lib, rig.activity(bufs["states"], 0, act))
    m.sync()
    a2 = m.download(act).copy()
    conv1, h1 = oracle_activations(rig.c, rig.unflat(after["p"]), batch["states"])
    s1, abs1, n1 = RD.per_unit(conv1, h1)
    tol = n1 * ACT_ATOL + ACT_RTOL * abs1
    assert np.all(np.abs(a2 - s1) <= tol), (row, float(np.max(np.abs(a2 - s1) / tol)))
    revived = s1[killed] > 0
    print("redo %s: %d of the %d killed units fire again after the recycle" % (row, int(revived.sum()), len(killed)))
    assert revived.any() and np.all(a2[np.asarray(killed)[revived]] > 0)
    rig.close()


# =============================================================================== 5: learning goes on
LEARN_CASES = {"d": dict(architecture="data-efficient", hidden=32), "c": dict(architecture="canonical", hidden=64)}
LEARN_DEFAULTS = dict(atoms=51, actions=6, multi_step=3, discount=0.99, v_min=-10.0, v_max=10.0, batch=4, history=4)
LEARN_SEEDS = {"d": 0, "c": 0}


def learn_check(lib, mem, case):
    """One learn step (rb_learner_learn + rb_learner_clip_adam, step 1) from a recycled state against learn_steps.OracleRun started from
    the same state, at helpers.assert_learn_trace_matches' tolerances; the update of every element against optimizer_scenarios'
    float64 one-step reference (check_update, m0 = v0 = 0 where recycled); a recycled outgoing weight, which starts at 0 with zero moments,
    moves by -lr g / (|g| + eps): at most lr, and lr to 1 % where |g| >= 100 eps."""
    cfgd = dict(LEARN_DEFAULTS, **LEARN_CASES[case])
    hy = scenarios.LEARN_HYPER
    assert (hy["lr"], hy["adam_eps"]) == (S.LR, S.EPS)
    inp = two_step_inputs(cfgd, LEARN_SEEDS[case])
    B, H = cfgd["batch"], cfgd["hidden"]
    name = "_redo_learn_" + case
    scenarios.LEARN_CONFIGS[name] = cfgd
    ad = CAbiLearnAdapter(lib, mem, name)
    try:
        ad.load(inp["online"], inp["target"])
        units = unit_layout(lib, ad.cfg)
        f = np.concatenate([[0], np.cumsum(units)])
        mask = np.zeros(int(f[-1]), np.uint8)
        for k, n in enumerate(units):
            mask[f[k] + np.arange(1, n, 5)] = 1                                         # a fifth of every layer
        mbuf = mem.upload(mask)
        L.check(lib, lib.rb_learner_recycle_units(ad.h, mem.ptr(mbuf), STD, SEED, DRAW, 1, mem.ptr(ad.adam_m), mem.ptr(ad.adam_v), mem.stream))
        mem.sync()
        dl = lambda b: np.array(mem.download(b.detach() if hasattr(b, "detach") else b), copy=True)
        p0, t0 = dl(ad.p_on), dl(ad.p_tg)
        before = dict(p=p0, m=dl(ad.adam_m), v=dl(ad.adam_v))
        st0 = dict(p=ad._flat(inp["online"]), t=ad._flat(inp["target"]), m=before["m"], v=before["v"])
        want, kind, _both = RD.recycle(ad.layout, st0, mask, STD, SEED, DRAW)
        assert np.array_equal(_bits(p0), _bits(want["p"])) and np.array_equal(_bits(t0), _bits(want["t"]))
        inp = dict(inp, online=ad._unflat(p0), target=ad._unflat(t0))
        stepper = OracleRun(inp)
        st = inp["steps"][0]
        ad.reset_noise_online(st["raw_on"])
        got = ad.learn_step(st["batch"], st["raw_tg"])
        conv_masks = [ad.debug(6 + i, shp, np.float32) > 0 for i, shp in enumerate(conv_shapes(inp["cfg"], B))]
        o = stepper.step(0, conv_masks=conv_masks)
        w = o["want"]
        print("redo learn %s: hidden ReLU margin %.3e, conv flips %s" % (case, w["hidden_relu_margin"], w["conv_flips"]))
        assert w["hidden_relu_margin"] >= RELU_MARGIN, "ill-conditioned seed: a hidden pre-activation within rounding noise of 0"
        assert all(ratio < 1.0 for _n, _a, ratio in w["conv_flips"]), w["conv_flips"]
        got_t = {"s0_loss": got["loss"], "s0_grad_norm": np.float32(got["grad_norm"])}
        want_t = {"s0_loss": w["loss"], "s0_grad_norm": np.float32(o["total"])}
        for n_ in o["clipped"]:
            got_t["s0_grad/" + n_], want_t["s0_grad/" + n_] = got["grads"][n_], o["clipped"][n_]
        for n_, p in ad.params().items():
            got_t["s0_param/" + n_], want_t["s0_param/" + n_] = p, o["params"][n_]
        assert_learn_trace_matches(got_t, want_t, label="redo learn " + case)
        after = dict(p=dl(ad.p_on), m=dl(ad.adam_m), v=dl(ad.adam_v))
        gp = dl(ad.grads)
        S.check_update("redo_" + case, before, after, gp, 1, "first Adam step after a recycle / " + case)
        # m0 = v0 = 0 at step 1: the update is -lr g / (|g| + eps) in exact arithmetic, i.e. -+lr wherever |g| >> eps and never more
        out0 = (kind == RD.OUTGOING) & (p0 == 0.0) & (np.abs(gp) >= 1e-30)
        assert out0.sum() > 100
        g8 = gp[out0].astype(np.float64)
        step, want_step = after["p"][out0].astype(np.float64), -S.LR * g8 / (np.abs(g8) + S.EPS)
        assert np.all(np.abs(step) <= S.LR * (1 + 1e-6)) and np.all(np.sign(step) == -np.sign(g8))
        np.testing.assert_allclose(step, want_step, rtol=1e-5, atol=1e-30, err_msg="first Adam step of a recycled outgoing weight")
        big = np.abs(g8) >= 100 * S.EPS
        print("redo learn %s: %d recycled outgoing weights with a gradient, largest |step| / lr %.4f, %d of them with |g| >= 100 eps"
              % (case, int(out0.sum()), float(np.abs(step).max() / S.LR), int(big.sum())))
        assert np.all(np.abs(step[big]) >= S.LR * 0.99)
    finally:
        ad.close()
        scenarios.LEARN_CONFIGS.pop(name, None)


def one_call_check(lib, mem):
    """The one-call path (rb_learner_train_step, the pass left pending) from a recycled state.  Twin A recycles through the library
    with a pass pending; twin B flushes and gets the oracle's result written by hand.  Two further steps: loss, parameters, target,
    moments, gradients and the replay's tree bit-identical, i.e. the recycle leaves no hidden state on that path."""
    c = DS.case_config("z51-a6")
    hs = [DS.ts_build(lib, mem, c, "_redo_oc%d" % i, flags=L.LEARNER_DEFER_UPDATE) for i in range(2)]
    try:
        for rp, ad, o, job in hs:
            DS.ts_call(lib, mem, c, rp, ad, o, job)
        units = unit_layout(lib, hs[0][1].cfg)
        mask = np.zeros(int(sum(units)), np.uint8)
        mask[::3] = 1
        rp, ad, o, job = hs[0]
        mbuf = mem.upload(mask)
        L.check(lib, lib.rb_learner_recycle_units(ad.h, mem.ptr(mbuf), STD, 9, 2 ** 32 + 1, 1, mem.ptr(ad.adam_m), mem.ptr(ad.adam_v), mem.stream))
        rp, ad, o, job = hs[1]
        L.check(lib, lib.rb_learner_flush(ad.h, mem.stream))
        s = DS.ts_state(mem, rp, ad, o)
        want, _kind, _both = RD.recycle(ad.layout, dict(p=s["params"], t=s["target"], m=s["m"], v=s["v"]), mask, STD, 9, 2 ** 32 + 1)
        for buf, key in ((ad.p_on, "p"), (ad.p_tg, "t"), (ad.adam_m, "m"), (ad.adam_v, "v")):
            _store(buf.detach() if hasattr(buf, "detach") else buf, want[key])
        mem.sync()
        a, b = DS.ts_state(mem, *hs[0][:3]), DS.ts_state(mem, *hs[1][:3])
        for k in ("params", "target", "m", "v"):
            assert DS.same_bits(a[k], b[k]), "right after the recycle: %s" % k
        for _ in range(2):
            for rp, ad, o, job in hs:
                DS.ts_call(lib, mem, c, rp, ad, o, job)
        for rp, ad, o, job in hs:
            L.check(lib, lib.rb_learner_flush(ad.h, mem.stream))
        a, b = DS.ts_state(mem, *hs[0][:3]), DS.ts_state(mem, *hs[1][:3])
        for k in a:
            assert DS.same_bits(a[k], b[k]), "two steps after the recycle the twins differ in %s" % k
        assert np.isfinite(a["loss"]).all()
    finally:
        for i, (rp, ad, o, job) in enumerate(hs):
            ad.close(); rp.close()
            DS.drop_config("_redo_oc%d" % i)
