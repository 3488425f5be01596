"""The optimiser pass (clip_grad_norm_ + Adam, agent.py:97-98) in every form the library runs it, against a float64 ONE-STEP
reference formed from the device's own state.  Shared by tests/test_optimizer_emu.py (NumpyMem, host interpreter) and
tests/test_optimizer_gpu.py (TorchMem).

The forms (adam_body.h, adam_kernels.h, grad_finish.h, optimizer_host.h):
  clip_grad         rb_learner_clip_grad: k_sumsq + k_clip_scale
  value / device    rb_learner_clip_adam, step by value / step = 0 (device counter): k_clip_adam<4, true, false>
  flush             RB_LEARNER_DEFER_UPDATE: rb_learner_clip_adam_deferred, then rb_learner_flush (twice)
  hosted            deferred, then attach + rb_replay_sample_fused_noise: rb_adam_hosted_block as workgroups of k_sample
  hosted25          the same behind a 25-transition window: rb_launch_adam_pending -> k_adam_pending, plain
  pairs_flush / pairs_hosted   RB_LEARNER_IMPLICIT_SIGMA: rb_adam_hosted_pairs through k_adam_pending / through k_sample
  fused_tile        RB_LEARNER_FUSE_FC_H_DW: k_clip_adam<4, true, true> with rb_fused_dw_adam_tile

The reference.  Before a pass p0, m0, v0, g (and the noise where a form needs it) are downloaded, after it p1, m1, v1, g1 and
the norm.  From the float32 values and the float32 scalars the host forms (w1 = (float)(1 - b1), b2, w2 = (float)(1 - b2),
s = (float)(-(lr / bc1)), r = (float)sqrt(bc2), eps) numpy computes in float64
    g' = fl32(g * coef)          coef = min(1, f32(max_norm) / (f32(norm_dev) + f32(1e-6))) re-formed in float32 from the DEVICE norm
    m  = m0 + w1 (g' - m0)       v = v0 b2 + (w2 g') g'       D = sqrt(v) / r + eps       delta = s m / D       p = p0 + delta
Every step starts from the device's own state, so nothing drifts and the bounds stay at rounding level for any number of steps.

Bounds, u = 2^-24 (half an ulp, relative), from the roundings of rb_adam_elem (built with -ffp-contract=off; sqrt and the two
divisions are the correctly rounded ones — the claim of adam_body.h that these bounds put to the test):
  norm   |norm_dev - norm64| <= 2e-6 norm64: the project's own figure (tests/test_learner_gpu.py).
  g      g' is ONE float32 product: bit-equal over the whole buffer when coef < 1, bit-unchanged when coef == 1.
  m      m1 = fl(w1 * fl(g' - m0) + m0), an fma: the subtraction errs by <= u |g' - m0| <= u (|g'| + |m0|), scaled by w1 < 1;
         the final rounding by <= u |m1| and |m1| <= max(|g'|, |m0|) (a convex combination).    |m1 - m| <= 2u (|g'| + |m0|) =: em
  v      v1 = fl(fl(v0 b2) + fl(fl(w2 g') g')): non-negative terms, each carrying at most three roundings on its path to the
         result, (1 + u)^3 - 1 < 4u.                                                          |v1 - v| <= 4u v
  p      D1 = fl(fl(fl(sqrt(v1)) / r) + eps): v1 within 4u of v -> sqrt within 2u, + u (sqrt) + u (division) + u (sum; both
         terms positive): D1 within 5u of D.  q1 = fl(m1 / D1): |q1 - m / D| <= em / D + (5u + u) |m / D|.  delta1 = fl(s q1):
         one more u: |delta1 - delta| <= |s| em / D + 7u |delta|; the eighth u absorbs the second-order terms.  p1 = fl(p0 +
         delta1): <= u |p1|.                               |p1 - p| <= u |p| + |s| em / D + 8u |delta|
No tuned constant.  Precondition, asserted: no intermediate of the reference lies in (0, 2^-126) — denormals are not the
subject; the generator keeps |g| in {0} U [1e-15, 1e3].

RATIOS collects the largest observed error / bound per (form, bound) for profiles/optimizer_bounds.txt."""
import ctypes as C
import math

import numpy as np

import scenarios
from cabi_adapter import CAbiLearnAdapter, CAbiReplayAdapter
from oracle import learner_oracle as O
from rainbow_amd import _lib as L
from ts_scenarios import ts_args, ts_build

U = 2.0 ** -24
TINY = 2.0 ** -126
B1, B2 = 0.9, 0.999
LR, EPS = scenarios.LEARN_HYPER["lr"], scenarios.LEARN_HYPER["adam_eps"]
NORM_RTOL = 2e-6
RATIOS = {}

STEPS = (1, 2, 10, 1000, 10 ** 6, 2 ** 32 + 3)


def _note(form, bound, ratio):
    RATIOS[(form, bound)] = max(RATIOS.get((form, bound), 0.0), float(ratio))


def format_ratios(title):
    lines = ["# %s: largest observed |error| / bound per form (a value above 1 fails the test)" % title]
    for (form, bound) in sorted(RATIOS):
        lines.append("%-14s %-5s %.4f" % (form, bound, RATIOS[(form, bound)]))
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------------------------------------ memory helpers --
def _store(buf, arr):
    """In-place write into caller-owned 'device' memory (numpy array or torch tensor)."""
    arr = np.ascontiguousarray(arr)
    if isinstance(buf, np.ndarray):
        buf[...] = arr.reshape(buf.shape)
    else:
        import torch
        buf.detach().copy_(torch.from_numpy(arr).reshape(buf.shape))


def _dl(mem, buf):
    return np.array(mem.download(buf.detach() if hasattr(buf, "detach") else buf), copy=True)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def state(rig):
    rig.mem.sync()
    ad = rig.ad
    return dict(p=_dl(rig.mem, ad.p_on), m=_dl(rig.mem, ad.adam_m), v=_dl(rig.mem, ad.adam_v), g=_dl(rig.mem, ad.grads))


def same_state(a, b, label, keys=("p", "m", "v", "g")):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (label, k)


# ----------------------------------------------------------------------------------------------------- reference --
def host_scalars(step):
    """The by-value scalars exactly as clip_adam_impl forms them (doubles, rounded once to float32)."""
    bc1, bc2 = 1.0 - math.pow(B1, float(step)), 1.0 - math.pow(B2, float(step))
    f = np.float32
    return dict(w1=f(1.0 - B1), b2=f(B2), w2=f(1.0 - B2), s=f(-(LR / bc1)), r=f(math.sqrt(bc2)), eps=f(EPS))


def clip_coef(norm_dev, max_norm):
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm_dev) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else np.float32(c)


def check_clip(form, g, g1, norm_dev, max_norm, label):
    """Norm, coefficient and the stored gradient.  Returns g' (float32)."""
    exact = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    if norm_dev is None:
        assert max_norm == float("inf")
        coef = np.float32(1.0)
    else:
        if exact == 0.0:
            assert float(norm_dev) == 0.0, (label, norm_dev)
        else:
            rel = abs(float(norm_dev) - exact) / exact
            _note(form, "norm", rel / NORM_RTOL)
            assert rel <= NORM_RTOL, (label, "norm", float(norm_dev), exact, rel)
        coef = clip_coef(norm_dev, max_norm)
        # the float64 norm alone decides whether the clip bites: every case keeps max_norm at least 1e-4 (50 x the norm
        # tolerance) away from the norm
        ratio = float(np.float32(max_norm)) / (exact + 1e-6)
        assert abs(ratio - 1.0) > 5e-5, (label, "the case must not sit on the clip threshold", ratio)
        assert bool(coef < 1.0) == (ratio < 1.0), (label, "clip decision", float(coef), ratio)
    if coef < 1.0:
        gp = (g * coef).astype(np.float32)
        assert np.array_equal(_bits(g1), _bits(gp)), (label, "stored gradient != fl32(g * coef)",
                                                      int(np.sum(_bits(g1) != _bits(gp))))
    else:
        gp = g
        assert np.array_equal(_bits(g1), _bits(g)), (label, "the gradient changed although the clip was idle")
    return gp


def check_update(form, before, after, gp, step, label):
    """m, v, p of one Adam step from `before` with the (clipped) gradient gp against the float64 reference."""
    k = {n: np.float64(x) for n, x in host_scalars(step).items()}
    g, m0, v0, p0 = (np.asarray(x, dtype=np.float64) for x in (gp, before["m"], before["v"], before["p"]))
    d = g - m0
    wd = k["w1"] * d
    m = m0 + wd
    vb, wg = v0 * k["b2"], k["w2"] * g
    wgg = wg * g
    v = vb + wgg
    rt = np.sqrt(v)
    sc = rt / k["r"]
    D = sc + k["eps"]
    q = m / D
    delta = k["s"] * q
    p = p0 + delta
    for name, x in (("g'", g), ("g'-m0", d), ("w1(g'-m0)", wd), ("m", m), ("v0 b2", vb), ("w2 g'", wg), ("w2 g' g'", wgg), ("v", v),
                    ("sqrt v", rt), ("sqrt v / r", sc), ("m / D", q), ("delta", delta), ("p", p)):
        ax = np.abs(x)
        assert not np.any((ax > 0) & (ax < TINY)), (label, "precondition: a denormal intermediate in", name)
    em = 2 * U * (np.abs(g) + np.abs(m0))
    bounds = dict(m=em, v=4 * U * v, p=U * np.abs(p) + np.abs(k["s"]) * em / D + 8 * U * np.abs(delta))
    got = dict(m=after["m"], v=after["v"], p=after["p"])
    want = dict(m=m, v=v, p=p)
    for name in ("m", "v", "p"):
        err = np.abs(got[name].astype(np.float64) - want[name])
        b = bounds[name]
        pos = b > 0
        assert np.all(err[~pos] == 0), (label, name, "must be exact where the bound is zero")
        ratio = float(np.max(err[pos] / b[pos])) if np.any(pos) else 0.0
        _note(form, name, ratio)
        assert ratio <= 1.0, (label, name, "error / bound", ratio, int(np.argmax(np.where(pos, err / np.where(pos, b, 1), 0))))
    return dict(m=m, v=v, p=p, delta=delta)


# ----------------------------------------------------------------------------------------------------- gradients --
def make_grad(layout, n, seed, pattern):
    """One seeded generator.  'scales': per-tensor scales 1e-8 .. 1e2 over the parameter layout; 'zeros': the same with whole
    tensors and interior ranges exactly zero; 'dominant': one element carries 99 % of the norm; 'allzero'."""
    if pattern == "allzero":
        return np.zeros(n, dtype=np.float32)
    rs = np.random.RandomState(seed)
    names = sorted(layout, key=lambda k: layout[k][0])
    exps = np.linspace(-8.0, -1.0 if pattern == "dominant" else 2.0, len(names))
    rs.shuffle(exps)
    scale = np.full(n, 1e-3)                                   # (floats no tensor covers: padding)
    for name, e in zip(names, exps):
        off, shape = layout[name]
        scale[off:off + int(np.prod(shape))] = 10.0 ** e
    z = rs.randn(n)
    z = np.where(z < 0, -1.0, 1.0) * np.clip(np.abs(z), 1e-3, 5.0)      # |g| >= 1e-3 x its tensor's scale: nothing near a denormal
    g = (z * scale).astype(np.float32)
    if pattern == "zeros":
        for name in names[::3]:
            off, shape = layout[name]
            g[off:off + int(np.prod(shape))] = 0.0
        g[1000:5000] = 0.0                                      # across a block boundary of the plain pass (4096 floats)
        g[60001:60007] = 0.0                                    # inside quads
    if pattern == "dominant":
        kbig = int(rs.randint(4097, n - 1))
        g[kbig] = 0.0
        rest = math.sqrt(float(np.sum(g.astype(np.float64) ** 2)))
        g[kbig] = np.float32(-rest * math.sqrt(0.9801 / 0.0199))          # 0.99 of the norm
    assert float(np.max(np.abs(g))) <= 1e3 and (not np.any(g != 0) or float(np.min(np.abs(g[g != 0]))) >= 1e-15)
    return g


def resolve_max_norm(kind, g):
    norm = math.sqrt(float(np.sum(g.astype(np.float64) ** 2)))
    if kind in ("inf", "inf_null"):
        return float("inf")
    if isinstance(kind, (int, float)):
        return float(np.float32(kind))
    # far from the norm on both sides, and one pair 1e-4 (50 x the norm tolerance) to either side of the threshold, which for
    # the kernel's coefficient is norm + 1e-6
    f = {"idle": 3.0, "bite": 0.3, "near_idle": 1.0 + 1e-4, "near_bite": 1.0 - 1e-4}[kind]
    return float(np.float32(f * (norm + 1e-6)))


# ---------------------------------------------------------------------------------------------------------- rigs --
class Rig:
    pass


def build_rig(lib, Mem, name, with_replay, flags=0):
    r = Rig()
    r.lib, r.name = lib, name
    if with_replay:
        r.mem, r.rp, r.ad, r.out, r.job = ts_build(lib, Mem, name)
    else:
        r.mem = Mem()
        r.rp = r.out = r.job = None
        r.ad = CAbiLearnAdapter(lib, r.mem, name)
        cfg = O.Config(**scenarios.LEARN_CONFIGS[name])
        r.ad.load(O.init_params(cfg, 1), O.init_params(cfg, 2))
    r.ctr = r.mem.upload(np.zeros(1, np.int64))
    L.check(lib, lib.rb_learner_set_step_counter(r.ad.h, r.mem.ptr(r.ctr)))
    L.check(lib, lib.rb_learner_set_flags(r.ad.h, flags))
    r.norm = r.mem.upload(np.full(1, -1.0, np.float32))
    return r


def close_rig(r):
    r.ad.close()
    if r.rp is not None:
        r.rp.close()


def _clip_adam(rig, fn, max_norm, step, norm_ptr):
    m, ad = rig.mem, rig.ad
    L.check(rig.lib, fn(ad.h, max_norm, m.ptr(ad.adam_m), m.ptr(ad.adam_v), LR, B1, B2, EPS, step, norm_ptr, m.stream))


def _sample(rig, job):
    m, o = rig.mem, rig.out
    B = scenarios.LEARN_CONFIGS[rig.name]["batch"]
    L.check(rig.lib, rig.lib.rb_replay_sample_fused_noise(rig.rp.h, B, 0.4, None, 64, m.ptr(o["tree_idx"]), None, None, m.ptr(o["actions"]),
                                                         m.ptr(o["returns"]), m.ptr(o["nonterm"]), m.ptr(o["weights"]), C.byref(job), m.stream))


def sampler_view(rig):
    m, o = rig.mem, rig.out
    m.sync()
    h = rig.rp.raw_header()
    return dict(idx=_dl(m, o["tree_idx"]), actions=_dl(m, o["actions"]), returns=_dl(m, o["returns"]), nonterm=_dl(m, o["nonterm"]),
                weights=_dl(m, o["weights"]), z_on=_dl(m, rig.ad.z_on), z_tg=_dl(m, rig.ad.z_tg), tree=rig.rp.tree().copy(),
                hdr=np.array([h.index, h.full, h.last_attempts, h.last_status, h.rng_counter], dtype=np.float64))


def run_synthetic(rig, form, g, max_norm, step, null_norm=False):
    """Write g into grads_dev, declare it modified, run one pass in `form`.  -> (before, after, norm or None, hosted flag)"""
    lib, m, ad = rig.lib, rig.mem, rig.ad
    _store(ad.grads, g)
    L.check(lib, lib.rb_learner_grads_modified(ad.h))
    _store(rig.ctr, np.array([step], np.int64))               # the caller owns the counter: the value, directly
    _store(rig.norm, np.full(1, -1.0, np.float32))
    before = state(rig)
    nptr = None if null_norm else m.ptr(rig.norm)
    hosted = None
    if form == "value":
        _clip_adam(rig, lib.rb_learner_clip_adam, max_norm, step, nptr)
    elif form == "device":
        _clip_adam(rig, lib.rb_learner_clip_adam, max_norm, 0, nptr)
    elif form == "flush":
        _clip_adam(rig, lib.rb_learner_clip_adam_deferred, max_norm, 0, nptr)
        L.check(lib, lib.rb_learner_flush(ad.h, m.stream))
        once = state(rig)
        L.check(lib, lib.rb_learner_flush(ad.h, m.stream))
        same_state(once, state(rig), "a second flush must change nothing")
    elif form == "hosted":
        _clip_adam(rig, lib.rb_learner_clip_adam_deferred, max_norm, 0, nptr)
        job_out = L.NoiseJob()
        hosted = lib.rb_learner_attach_pending(ad.h, C.byref(rig.job), scenarios.LEARN_CONFIGS[rig.name]["batch"], C.byref(job_out))
        assert hosted in (0, 1), lib.rb_last_error()
        _sample(rig, job_out)
        L.check(lib, lib.rb_learner_pending_launched(ad.h))
    else:
        raise ValueError(form)
    after = state(rig)
    norm = None if null_norm else np.float32(_dl(m, rig.norm)[0])
    return before, after, norm, hosted


def check_synthetic(rig, form, label_form, g, kind, step, label):
    max_norm = resolve_max_norm(kind, g)
    before, after, norm, hosted = run_synthetic(rig, form, g, max_norm, step, null_norm=(kind == "inf_null"))
    assert np.array_equal(_bits(before["g"]), _bits(g))
    gp = check_clip(label_form, g, after["g"], norm, max_norm, label)
    check_update(label_form, before, after, gp, step, label)
    return after, norm, hosted


# The synthetic cases of the form group: every step number, every gradient pattern, every kind of max_norm
CASES = (("scales", "idle", 1), ("zeros", "bite", 2), ("dominant", "near_idle", 10), ("dominant", "near_bite", 1000),
         ("scales", "inf", 10 ** 6), ("zeros", "inf_null", 2 ** 32 + 3), ("allzero", 10.0, 2 ** 32 + 3), ("scales", "bite", 2 ** 32 + 3))


def form_group_check(lib, Mem, monkeypatch, cases=CASES, name="dataeff"):
    """Forms 2 to 5 on the same inputs: rb_learner_clip_adam by value and by device counter, deferred + flush, deferred + hosted
    by the sampler launch, deferred + the pending pass as a launch of its own (window 25).  Each against the reference, all
    bit-identical in p, m, v, g and the norm; the hosting samplers' own outputs equal those of twins that host nothing."""
    n25 = name + "-n21"
    monkeypatch.setitem(scenarios.LEARN_CONFIGS, n25, dict(scenarios.LEARN_CONFIGS[name], multi_step=21))
    monkeypatch.setenv("RB_OPTS", "spec_draw=0")
    D = L.LEARNER_DEFER_UPDATE
    rigs = dict(device=build_rig(lib, Mem, name, True), value=build_rig(lib, Mem, n25, True), flush=build_rig(lib, Mem, name, False, D),
                hosted=build_rig(lib, Mem, name, True, D), hosted25=build_rig(lib, Mem, n25, True, D))
    assert rigs["hosted25"].rp.bufs.window_len == 25 and rigs["hosted"].rp.bufs.window_len <= 24
    layout, n = rigs["device"].ad.layout, rigs["device"].ad.n_params
    seen_steps = set()
    for ci, (pattern, kind, step) in enumerate(cases):
        g = make_grad(layout, n, 100 + ci, pattern)
        outs = {}
        for fname, rig in rigs.items():
            form = {"hosted25": "hosted"}.get(fname, fname)
            label = "%s/%s/%s/step %d" % (fname, pattern, kind, step)
            after, norm, hosted = check_synthetic(rig, form, fname, g, kind, step, label)
            if form == "hosted":          # (max_norm = inf without a norm buffer needs no partials and is never left pending)
                assert hosted == (0 if kind == "inf_null" else 1), label
            elif rig.rp is not None:      # the twin that hosts nothing: the same sampler call with the plain job
                _sample(rig, rig.job)
            outs[fname] = (after, norm)
        if pattern == "allzero":          # the norm is 0, the coefficient clamps to 1, the parameters move by momentum alone
            assert float(outs["device"][1]) == 0.0
        for fname in rigs:
            same_state(outs["device"][0], outs[fname][0], ("form group", ci, fname))
            assert outs[fname][1] is None or _bits(outs[fname][1]) == _bits(outs["device"][1]), (ci, fname, "norm")
        for host, twin in (("hosted", "device"), ("hosted25", "value")):
            a, b = sampler_view(rigs[host]), sampler_view(rigs[twin])
            for k in a:
                assert np.array_equal(a[k], b[k]), (ci, host, "sampler output", k)
        seen_steps.add(step)
    for rig in rigs.values():
        close_rig(rig)
    return seen_steps


def trajectory_check(lib, Mem, monkeypatch, steps=50, name="dataeff", forms=("value", "hosted")):
    """`steps` consecutive passes, another gradient pattern and another max_norm every step, each checked one-step from the
    device's own state; the forms bit-identical after every step."""
    monkeypatch.setenv("RB_OPTS", "spec_draw=0")
    rigs = {f: build_rig(lib, Mem, name, f == "hosted", L.LEARNER_DEFER_UPDATE if f in ("hosted", "flush") else 0) for f in forms}
    first = rigs[forms[0]]
    patterns = ("scales", "zeros", "dominant", "scales", "allzero")
    kinds = ("idle", "bite", "near_bite", "inf", "near_idle", "bite")
    for t in range(1, steps + 1):
        pattern, kind = patterns[t % len(patterns)], kinds[t % len(kinds)]
        if pattern == "allzero":
            kind = 10.0
        g = make_grad(first.ad.layout, first.ad.n_params, 1000 + t, pattern)
        outs = [check_synthetic(rigs[f], f, f, g, kind, t, "trajectory/%s/step %d/%s/%s" % (f, t, pattern, kind))[0] for f in forms]
        for f, o in zip(forms[1:], outs[1:]):
            same_state(outs[0], o, ("trajectory", t, f))
    for rig in rigs.values():
        close_rig(rig)


CLIP_GRAD_CASES = (("scales", "idle"), ("zeros", "bite"), ("dominant", "near_idle"), ("dominant", "near_bite"), ("scales", "inf"),
                   ("allzero", 10.0))


def clip_grad_check(lib, Mem, name="dataeff", cases=CLIP_GRAD_CASES):
    """Form 1, rb_learner_clip_grad: k_sumsq + k_clip_scale on synthetic gradients, then once more on the partials a learn call
    left (no k_sumsq pass; from 1 M parameters on the scale kernel is capped at 256 blocks: the canonical shape of the GPU file)."""
    rig = build_rig(lib, Mem, name, False)
    m, ad = rig.mem, rig.ad
    for ci, (pattern, kind) in enumerate(cases):
        g = make_grad(ad.layout, ad.n_params, 300 + ci, pattern)
        max_norm = resolve_max_norm(kind, g)
        _store(ad.grads, g)
        L.check(lib, lib.rb_learner_grads_modified(ad.h))
        _store(rig.norm, np.full(1, -1.0, np.float32))
        before = state(rig)
        L.check(lib, lib.rb_learner_clip_grad(ad.h, max_norm, m.ptr(rig.norm), m.stream))
        after = state(rig)
        check_clip("clip_grad", g, after["g"], np.float32(_dl(m, rig.norm)[0]), max_norm, "clip_grad/%s/%s" % (pattern, kind))
        same_state(before, after, "clip_grad touches the gradient only", keys=("p", "m", "v"))
    c = scenarios.LEARN_CONFIGS[name]
    rs = np.random.RandomState(12)
    draws = O.noise_draw_count(O.Config(**c))
    ad.reset_noise_online(rs.randn(draws).astype(np.float32))
    # (a learn call writes the tensors of the layout, not the alignment gaps between them, and its partials cover what it wrote:
    # the gaps must hold the zeros of a freshly allocated buffer again, not the synthetic values k_sumsq has just summed)
    _store(ad.grads, np.zeros(ad.n_params, np.float32))
    for kind in ("bite", "idle"):
        ad.learn_only(scenarios.make_batch(c, 31), rs.randn(draws).astype(np.float32))
        g = state(rig)["g"]
        assert np.any(g != 0)
        max_norm = resolve_max_norm(kind, g)
        L.check(lib, lib.rb_learner_clip_grad(ad.h, max_norm, m.ptr(rig.norm), m.stream))
        check_clip("clip_grad", g, state(rig)["g"], np.float32(_dl(m, rig.norm)[0]), max_norm, "clip_grad/learn partials/" + kind)
    close_rig(rig)


def single_form_check(lib, Mem, name, form, cases):
    """One form alone at another shape (the canonical network: other block and norm-partial counts)."""
    rig = build_rig(lib, Mem, name, False)
    for ci, (pattern, kind, step) in enumerate(cases):
        g = make_grad(rig.ad.layout, rig.ad.n_params, 500 + ci, pattern)
        check_synthetic(rig, form, form, g, kind, step, "%s/%s/%s/%s/step %d" % (name, form, pattern, kind, step))
    close_rig(rig)


# --------------------------------------------------------------------------------------------- (mu, sigma) pairs --
def _hidden_ranges(ad):
    """[(mu offset, sigma offset, rows, cols, eps_in name, eps_out name)] of the hidden layer's two streams."""
    out = []
    for s in ("fc_h_v", "fc_h_a"):
        mu, shape = ad.layout[s + ".weight_mu"]
        sg, _ = ad.layout[s + ".weight_sigma"]
        out.append((mu, sg, shape[0], shape[1], s + ".eps_in", s + ".eps_out"))
    return out


def sigma_product(ad, g, noise, noise_layout):
    """g with the hidden layer's sigma-weight range replaced by g_mu * fl(eps_out[row] * eps_in[col]), in float32 as the
    backward and the pair pass form it; rows of the second stream take the second stream's eps_in."""
    g = g.copy()
    for mu, sg, rows, cols, ein, eout in _hidden_ranges(ad):
        ei = noise[noise_layout[ein][0]:noise_layout[ein][0] + cols].astype(np.float32)
        eo = noise[noise_layout[eout][0]:noise_layout[eout][0] + rows].astype(np.float32)
        prod = (eo[:, None] * ei[None, :]).astype(np.float32)
        g[sg:sg + rows * cols] = (g[mu:mu + rows * cols].reshape(rows, cols) * prod).astype(np.float32).ravel()
    return g


def plan_reports_implicit_sigma(lib, name, opts, flags):
    cfg = scenarios.LEARN_CONFIGS[name]
    from cabi_adapter import learner_config
    lc = learner_config(cfg)
    buf = C.create_string_buffer(1 << 14)
    L.check(lib, lib.rb_debug_launch_plan(C.byref(lc), opts.encode() if opts else None, 256, flags, 1, 1, buf, 1 << 14))
    return "implicit_sigma=1" in buf.value.decode()


def pairs_check(lib, Mem, monkeypatch, name="dataeff", opts="implicit_small=1,spec_draw=0"):
    """Form 6: a real rb_learner_train_step under DEFER_UPDATE | IMPLICIT_SIGMA leaves the (mu, sigma) pair pass pending; rig a
    runs it by rb_learner_flush (k_adam_pending), rig b by attach + a sampler launch whose noise job resamples BOTH nets (the
    online noise is overwritten by the launch that hosts the pass: only the snapshot gives the right sigma gradient)."""
    flags = L.LEARNER_DEFER_UPDATE | L.LEARNER_IMPLICIT_SIGMA
    if opts:
        monkeypatch.setenv("RB_OPTS", opts)
    else:
        monkeypatch.delenv("RB_OPTS", raising=False)
    assert plan_reports_implicit_sigma(lib, name, opts, flags), "the shape must take the implicit sigma gradient"
    a, b = build_rig(lib, Mem, name, True, flags), build_rig(lib, Mem, name, True, flags)
    from cabi_adapter import query_layout
    nl = query_layout(lib, a.ad.cfg, lib.rb_learner_noise_layout)
    sig = [(sg, sg + rows * cols) for _, sg, rows, cols, _, _ in _hidden_ranges(a.ad)]
    B = scenarios.LEARN_CONFIGS[name]["batch"]
    for rnd, max_norm in enumerate((10.0, 1e-3)):
        res = {}
        for tag, rig in (("pairs_flush", a), ("pairs_hosted", b)):
            m, ad = rig.mem, rig.ad
            ts = ts_args(name, m, rig.rp, ad, rig.out, rig.job, 0.4, 0, max_norm)
            ts.norm_dev = m.ptr(rig.norm)
            L.check(lib, lib.rb_learner_train_step(ad.h, C.byref(ts), m.stream))
            before = state(rig)                                   # (the pass is pending: grads_dev lacks this step's sigma range)
            noise = _dl(m, ad.z_on)
            step = int(_dl(m, rig.ctr)[0])
            assert step == rnd + 1
            g = sigma_product(ad, before["g"], noise, nl)
            assert any(not np.array_equal(g[lo:hi], before["g"][lo:hi]) for lo, hi in sig)
            job2 = L.NoiseJob()
            L.check(lib, lib.rb_learner_noise_job(ad.h, 2, C.byref(job2)))
            if tag == "pairs_flush":
                L.check(lib, lib.rb_learner_flush(ad.h, m.stream))
                mid = state(rig)
                _sample(rig, job2)                                # the twin sampler launch that hosts nothing
            else:
                job_out = L.NoiseJob()
                assert lib.rb_learner_attach_pending(ad.h, C.byref(job2), B, C.byref(job_out)) == 1
                _sample(rig, job_out)
                L.check(lib, lib.rb_learner_pending_launched(ad.h))
                mid = state(rig)
                assert not np.array_equal(_dl(m, ad.z_on), noise), "the hosting launch must have overwritten the online noise"
            norm = np.float32(_dl(m, rig.norm)[0])
            label = "%s/max_norm %g" % (tag, max_norm)
            bites = max_norm < 1.0
            if bites:
                assert float(norm) > max_norm, (label, "the clip must bite", float(norm))
                gp = check_clip(tag, g, mid["g"], norm, max_norm, label)     # the whole stored gradient, sigma range included
            else:
                gp = g
                assert clip_coef(norm, max_norm) == 1.0
                exact = math.sqrt(float(np.sum(g.astype(np.float64) ** 2)))
                rel = abs(float(norm) - exact) / exact
                _note(tag, "norm", rel / NORM_RTOL)
                assert rel <= NORM_RTOL, (label, "norm", rel)
            check_update(tag, before, mid, gp, step, label)
            L.check(lib, lib.rb_learner_flush(ad.h, m.stream))
            end = state(rig)
            same_state(mid, end, (label, "flush after the pass"), keys=("p", "m", "v"))
            assert np.array_equal(_bits(end["g"]), _bits(gp)), (label, "the stored gradient after flush")
            res[tag] = (end, norm, sampler_view(rig))
        same_state(res["pairs_flush"][0], res["pairs_hosted"][0], ("pairs: flush against hosted", max_norm))
        assert _bits(res["pairs_flush"][1]) == _bits(res["pairs_hosted"][1])
        for k in res["pairs_flush"][2]:
            assert np.array_equal(res["pairs_flush"][2][k], res["pairs_hosted"][2][k]), ("pairs: sampler output", k)
    close_rig(a); close_rig(b)


# ---------------------------------------------------------------------------------------------------- fused tile --
def fused_tile_check(lib, Mem, name="dataeff", bite=1e-3):
    """Form 7: learn under FUSE_FC_H_DW | WRITE_FUSED_GRADS, then rb_learner_clip_adam: the hidden layer's weight gradient exists
    only inside the pass, so the gradient it stored IS g' there; elsewhere g' = fl32(g * coef) as in every other form."""
    rig = build_rig(lib, Mem, name, False, L.LEARNER_FUSE_FC_H_DW | L.LEARNER_WRITE_FUSED_GRADS)
    m, ad = rig.mem, rig.ad
    c = scenarios.LEARN_CONFIGS[name]
    cfg = O.Config(**c)
    online, target = O.init_params(cfg, 1), O.init_params(cfg, 2)      # what build_rig loaded
    hid = np.zeros(ad.n_params, dtype=bool)
    for mu, sg, rows, cols, _, _ in _hidden_ranges(ad):
        hid[mu:mu + rows * cols] = True
        hid[sg:sg + rows * cols] = True
    rs = np.random.RandomState(21)
    draws = O.noise_draw_count(cfg)
    for step, max_norm in ((1, bite), (2, 10.0)):
        raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
        ad.reset_noise_online(raw_on)
        batch = scenarios.make_batch(c, 40 + step)
        ad.learn_only(batch, raw_tg)
        before = state(rig)
        _clip_adam(rig, lib.rb_learner_clip_adam, max_norm, step, m.ptr(rig.norm))
        after = state(rig)
        norm = np.float32(_dl(m, rig.norm)[0])
        label = "fused_tile/max_norm %g" % max_norm
        coef = clip_coef(norm, max_norm)
        gp = after["g"]
        rest = (before["g"][~hid] * coef).astype(np.float32) if coef < 1.0 else before["g"][~hid]
        assert np.array_equal(_bits(gp[~hid]), _bits(rest)), (label, "stored gradient outside the hidden layer")
        assert np.any(gp[hid] != 0)
        if coef < 1.0:
            assert step == 1 and float(norm) > max_norm
            want = O.learn(cfg, online, target, O.make_noise(cfg, raw_on), O.make_noise(cfg, raw_tg), batch)
            total, clipped = O.clip_grads(want["grads"], max_norm)
            np.testing.assert_allclose(float(norm), total, rtol=5e-5, atol=1e-7, err_msg=label)
            got = ad._unflat(gp)
            for k, w in clipped.items():                   # the tolerances of helpers.assert_learn_trace_matches
                np.testing.assert_allclose(got[k], w, rtol=2e-4, atol=5e-6 * float(np.max(np.abs(w))) + 1e-12, err_msg=label + " " + k)
        else:
            exact = math.sqrt(float(np.sum(gp.astype(np.float64) ** 2)))
            rel = abs(float(norm) - exact) / exact
            _note("fused_tile", "norm", rel / NORM_RTOL)
            assert rel <= NORM_RTOL, (label, "norm", rel)
        check_update("fused_tile", before, after, gp, step, label)
    close_rig(rig)


# ------------------------------------------------------------------------------------------------ skipped update --
def skipped_update_check(lib, Mem, name="dataeff"):
    """Form 8: the batch behind the gradient was a failed draw (the 16-slot ring of scenarios.sampler_gives_up_check as the
    learner's priority sink).  Under DEFER_UPDATE the pending pass — hosted by the next sampler launch, then by flush — must
    leave p, m, v, g bit-unchanged and write norm 0: the batch-status path of rb_adam_hosted_prologue and of k_clip_adam."""
    rig = build_rig(lib, Mem, name, False, L.LEARNER_DEFER_UPDATE)
    m, ad = rig.mem, rig.ad
    c = scenarios.LEARN_CONFIGS[name]
    B = c["batch"]
    rp = CAbiReplayAdapter(lib, m, 16, 4, 3, 0.99, 0.5)
    rs = np.random.RandomState(0)
    for _ in range(16):
        rp.append(scenarios.synth_state(rs, 4, 0), 1, 0.0, False)
    out = dict(tree_idx=m.empty((B,), np.int64), actions=m.empty((B,), np.int64), returns=m.empty((B,), np.float32),
               nonterm=m.empty((B,), np.float32), weights=m.upload(np.full(B, 7.0, np.float32)))
    L.check(lib, lib.rb_learner_set_priority_sink(ad.h, rp.h, m.ptr(out["tree_idx"])))
    job = L.NoiseJob()
    L.check(lib, lib.rb_learner_noise_job(ad.h, 1, C.byref(job)))

    def draw(job_):
        L.check(lib, lib.rb_replay_sample_fused_noise(rp.h, B, 0.5, None, 12, m.ptr(out["tree_idx"]), None, None, m.ptr(out["actions"]),
                                                     m.ptr(out["returns"]), m.ptr(out["nonterm"]), m.ptr(out["weights"]), C.byref(job_), m.stream))
    draw(job)
    m.sync()
    assert rp.raw_header().last_status == 1, "the scenario needs a draw that gives up"
    assert np.array_equal(_dl(m, out["weights"]), np.zeros(B, np.float32))
    _store(ad.adam_m, np.full(ad.n_params, 0.25, np.float32))      # an un-skipped pass WOULD move everything
    _store(ad.adam_v, np.full(ad.n_params, 1e-4, np.float32))
    draws = O.noise_draw_count(O.Config(**c))
    ad.reset_noise_online(rs.randn(draws).astype(np.float32))
    batch = scenarios.make_batch(c, 17)
    batch["weights"] = np.zeros(B, np.float32)                     # what the sampler wrote
    ad.learn_only(batch, rs.randn(draws).astype(np.float32))       # its head kernel copies the failed status
    m.sync()
    assert int(_dl(m, rig.ctr)[0]) == 0, "a failed batch must not advance the step number"
    g = make_grad(ad.layout, ad.n_params, 700, "scales")           # (nor may a gradient somebody put there be clipped)
    for how in ("hosted", "flush"):
        _store(ad.grads, g)
        L.check(lib, lib.rb_learner_grads_modified(ad.h))
        _store(rig.norm, np.full(1, -1.0, np.float32))
        before = state(rig)
        _clip_adam(rig, lib.rb_learner_clip_adam_deferred, 1e-3, 0, m.ptr(rig.norm))
        if how == "hosted":
            job_out = L.NoiseJob()
            assert lib.rb_learner_attach_pending(ad.h, C.byref(job), B, C.byref(job_out)) == 1
            draw(job_out)
            L.check(lib, lib.rb_learner_pending_launched(ad.h))
        else:
            L.check(lib, lib.rb_learner_flush(ad.h, m.stream))
        same_state(before, state(rig), ("skipped update", how))
        assert float(_dl(m, rig.norm)[0]) == 0.0, (how, "the skipped pass reports norm 0")
    L.check(lib, lib.rb_learner_set_priority_sink(ad.h, None, None))
    close_rig(rig)
    rp.close()
