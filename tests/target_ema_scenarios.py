"""The target network's EMA inside the optimiser pass (rb_learner_set_target_tau; adam_body.h rb_ema_elem), in every form the pass
runs in.  Shared by tests/test_target_ema_emu.py (NumpyMem, host interpreter) and tests/test_target_ema_gpu.py (TorchMem).

The rule, on the freshly written parameter p1:  tau == 1: t1 = p1 (t is not read);  otherwise t1 = fmaf(tau, p1 - t0, t0).

What every form is held to:
  (i)   p, m, v, the stored gradient and the norm are BIT-identical to the same pass with tau = 0 on copies of the same state;
  (ii)  tau == 1: t1 is bit-equal to p1;
  (iii) otherwise, in float64 from the device's p1 and the old target t0, with tau the float32 the C ABI carries:
            |t1 - (t0 + tau (p1 - t0))| <= u (tau |p1 - t0| + |t1|),     u = 2^-24
        fl(p1 - t0) = (p1 - t0)(1 + e), |e| <= u, reaches the result scaled by tau; the fma rounds once more, by at most u |t1|.
        No tuned constant.  Precondition, asserted: no intermediate of the reference lies in (0, 2^-126);
  (iv)  the targets of different forms on the same inputs are bit-identical to one another;
  a failed draw (batch status != 0) leaves the target bit-unchanged, like p, m and v.

Forms: `value` / `device` k_clip_adam<4, true, false, true>, `flush` the same kernel as the pending pass, `hosted` k_sample<1024, 4, true>,
`hosted25` k_adam_pending_ema behind a 25-transition window, `pairs_flush` / `pairs_hosted` rb_adam_hosted_pairs<true> through
k_adam_pending_ema / k_sample, `fused_tile` k_clip_adam<4, true, true> followed by k_target_ema, and rb_debug_adam_pass_ema
(optimizer_host.h, tests only: form 0 k_clip_adam, form 1 k_adam_pending_ema) at lengths the learner's own buffers never have.

RATIOS collects the largest observed error / bound of (iii) per (form, tau) for profiles/optimizer_bounds.txt."""
import ctypes as C

import numpy as np

import optimizer_scenarios as S
import scenarios
from cabi_adapter import CAbiReplayAdapter
from oracle import learner_oracle as O
from rainbow_amd import _lib as L
from ts_scenarios import ts_args

F32 = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -126
TAUS = (1.0, 0.5, 0.005, 2.0 ** -20)
SLACK = 4                     # floats behind every synthetic buffer: nothing may be written there
SENTINEL = F32(-777.25)
RATIOS = {}


def declare(lib):
    """argtypes of the two tests-only entries (neither is in include/rainbow_hip.h)."""
    vp = C.c_void_p
    base = [C.c_int32, vp, vp, vp, vp, C.c_int64, vp, C.c_int32, C.c_float, vp, vp, C.c_int64, C.c_double, C.c_double, C.c_double,
            C.c_double, vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, vp, vp, vp, vp]
    lib.rb_debug_adam_pass.restype = C.c_int
    lib.rb_debug_adam_pass.argtypes = base + [vp]
    lib.rb_debug_adam_pass_ema.restype = C.c_int
    lib.rb_debug_adam_pass_ema.argtypes = base + [vp, C.c_float, vp]
    return lib


def format_ratios(title):
    lines = ["# target EMA, %s: largest observed |t1 - (t0 + tau (p1 - t0))| / (u (tau |p1 - t0| + |t1|)) per form and tau "
             "(a value above 1 fails the test; tau = 1 is compared bit for bit and has no ratio)" % title]
    for (form, tau) in sorted(RATIOS):
        lines.append("%-14s tau %-12.6g %.4f" % (form, tau, RATIOS[(form, tau)]))
    return "\n".join(lines) + "\n"


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def check_target(form, tau, t0, p1, t1, label):
    """(ii) / (iii)."""
    if tau == 1.0:
        assert np.array_equal(_bits(t1), _bits(p1)), (label, "tau = 1: the target must equal the new parameters bit for bit",
                                                      int(np.sum(_bits(t1) != _bits(p1))))
        return
    tf = float(F32(tau))
    t0d, p1d, t1d = (np.asarray(x, dtype=np.float64) for x in (t0, p1, t1))
    d = p1d - t0d
    want = t0d + tf * d
    for name, x in (("p1 - t0", d), ("tau (p1 - t0)", tf * d), ("t", want)):
        ax = np.abs(x)
        assert not np.any((ax > 0) & (ax < TINY)), (label, "precondition: a denormal intermediate in", name)
    bound = U * (tf * np.abs(d) + np.abs(t1d))
    err = np.abs(t1d - want)
    pos = bound > 0
    assert np.all(err[~pos] == 0), (label, "must be exact where the bound is zero")
    ratio = float(np.max(err[pos] / bound[pos])) if np.any(pos) else 0.0
    print("target EMA %-40s tau %-12.6g error / bound %.4f" % (label, tau, ratio))
    RATIOS[(form, tau)] = max(RATIOS.get((form, tau), 0.0), ratio)
    assert ratio <= 1.0, (label, "target error / bound", ratio)
    assert not np.array_equal(_bits(t1), _bits(t0)) or not np.any(d != 0), (label, "the target did not move")


# ------------------------------------------------------------------------------------- synthetic buffers of any length --
def run_pass(lib, mem, form, st, parts, max_norm, step, status, pair=None, tau=0.0):
    """One pass through rb_debug_adam_pass (tau == 0) or rb_debug_adam_pass_ema over uploaded copies of st's p, g, m, v, t, each
    followed by SLACK sentinel floats that must survive.  -> (arrays after, norm, the pair pass's clipped word)."""
    n = st["p"].size
    dev = {k: mem.upload(np.concatenate([st[k].astype(F32), np.full(SLACK, SENTINEL, F32)])) for k in "pgmvt"}
    part, norm = mem.upload(np.asarray(parts, F32)), mem.upload(np.full(1, -1.0, F32))
    ctr, stat = mem.upload(np.array([step], np.int64)), mem.upload(np.array([status, 0, 0, 0], np.int32))
    clipped, args = mem.upload(np.full(4, -1, np.int32)), mem.upload(np.zeros(32, np.int64))
    pr = [0, 0, 0, 0, None, None, None]
    keep = []
    if pair is not None and form == 1:
        keep = [mem.upload(pair["eout"]), mem.upload(pair["ein"])]
        pr = [pair["mu4"], pair["len4"], pair["f4"], pair["split_row"], mem.ptr(keep[0]), mem.ptr(keep[1]), mem.ptr(clipped)]
    base = [form, mem.ptr(dev["p"]), mem.ptr(dev["g"]), mem.ptr(dev["m"]), mem.ptr(dev["v"]), n, mem.ptr(part), len(parts), max_norm,
            mem.ptr(norm), mem.ptr(ctr), step, S.LR, S.B1, S.B2, S.EPS, mem.ptr(stat), *pr, mem.ptr(args)]
    if tau == 0.0:
        L.check(lib, lib.rb_debug_adam_pass(*base, mem.stream))
    else:
        L.check(lib, lib.rb_debug_adam_pass_ema(*base, mem.ptr(dev["t"]), tau, mem.stream))
    mem.sync()
    out = {}
    for k in "pgmvt":
        a = np.array(mem.download(dev[k]), copy=True)
        assert np.array_equal(_bits(a[n:]), _bits(np.full(SLACK, SENTINEL, F32))), ("a store behind the end of", k, n, form, tau)
        out[k] = a[:n]
    return out, F32(mem.download(norm)[0]), int(mem.download(clipped)[0])


def make_state(n, seed):
    rs = np.random.RandomState(seed)
    return dict(p=rs.randn(n).astype(F32), g=(1e-2 * rs.randn(n)).astype(F32), m=(1e-3 * rs.randn(n)).astype(F32),
                v=(1e-4 * rs.rand(n)).astype(F32), t=rs.randn(n).astype(F32))


def same(a, b, label, keys="pgmv"):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (label, k, int(np.sum(_bits(a[k]) != _bits(b[k]))))


# n (floats): the tail alone (no whole quad), one quad and a tail, fewer quads than a block of 1024 with a 3-element tail,
# 4 x 1024 + 1 quads (the fifth block holds one quad)
PLAIN_SHAPES = (1, 3, 5, 4 * 700 + 3, 4 * (4 * 1024 + 1))


def plain_shapes_check(lib, Mem, n, taus=TAUS):
    """rb_debug_adam_pass_ema, forms 0 and 1, on a buffer of n floats: (i) against the same form with tau = 0, (ii) / (iii), (iv)
    form 0 against form 1, for a clip that bites and an idle one; and the failed draw."""
    from test_hosted_pass_order import make_parts, max_norm_for
    mem = Mem()
    st = make_state(n, 100 + n % 97)
    for bite in (True, False):
        parts = make_parts(257 if bite else 4097, 7 + int(bite))
        mx, step = max_norm_for(parts, bite), (7 if bite else 2 ** 32 + 3)
        plain = {form: run_pass(lib, mem, form, st, parts, mx, step, 0) for form in (0, 1)}
        assert (float(plain[0][1]) > mx) == bite
        assert not np.array_equal(_bits(plain[0][0]["p"]), _bits(st["p"]))
        for form in (0, 1):
            assert np.array_equal(_bits(plain[form][0]["t"]), _bits(st["t"])), "tau = 0 must leave the target alone"
        for tau in taus:
            got = {form: run_pass(lib, mem, form, st, parts, mx, step, 0, tau=tau) for form in (0, 1)}
            for form in (0, 1):
                label = "debug form %d / n %d / bite %s" % (form, n, bite)
                same(plain[form][0], got[form][0], (label, tau, "(i)"))
                assert _bits(got[form][1]) == _bits(plain[form][1]), (label, "norm")
                check_target("debug%d" % form, tau, st["t"], got[form][0]["p"], got[form][0]["t"], label)
            same(got[0][0], got[1][0], ("(iv) n %d" % n, tau), keys="pgmvt")
    for form in (0, 1):
        for tau in (1.0, 0.5):
            got, norm, _ = run_pass(lib, mem, form, st, make_parts(300, 3), 1e-3, 9, 1, tau=tau)
            same(st, got, ("failed draw", form, n, tau), keys="pgmvt")
            assert float(norm) == 0.0


def pair_shapes_check(lib, Mem, taus=TAUS):
    """The pair case of tests/test_hosted_pass_order.py (a hole that starts inside the second plain block, a pair range of two whole
    pair workgroups and one of 59 quads, a 2-element tail) through k_adam_pending_ema; reference: k_clip_adam with the EMA on the
    materialised gradient."""
    from test_hosted_pass_order import make_parts, max_norm_for, pair_case, pair_sigma
    mem = Mem()
    n, pair = pair_case()
    st = make_state(n, 3)
    g_full, (slo, shi) = pair_sigma(st, pair)
    st["g"][slo:shi] = 123.0                     # the pair pass never reads the sigma gradient
    parts = make_parts(300, 31)
    for bite in (True, False):
        mx = max_norm_for(parts, bite)
        plain, pnorm, pclipped = run_pass(lib, mem, 1, st, parts, mx, 5, 0, pair)
        assert (float(pnorm) > mx) == bite and pclipped == (1 if bite else 0)
        assert np.array_equal(_bits(plain["t"]), _bits(st["t"]))
        for tau in taus:
            got, norm, clipped = run_pass(lib, mem, 1, st, parts, mx, 5, 0, pair, tau=tau)
            label = "debug pairs / bite %s" % bite
            same(plain, got, (label, tau, "(i)"))
            assert _bits(norm) == _bits(pnorm) and clipped == pclipped
            check_target("debug_pairs", tau, st["t"], got["p"], got["t"], label)
            ref, _, _ = run_pass(lib, mem, 0, dict(st, g=g_full), parts, mx, 5, 0, tau=tau)
            same(ref, got, ("(iv) pairs against k_clip_adam", bite, tau), keys="pmvt")
    for tau in (1.0, 0.5):
        got, norm, clipped = run_pass(lib, mem, 1, st, parts, 1e-3, 9, 1, pair, tau=tau)
        same(st, got, ("failed draw, pairs", tau), keys="pgmvt")
        assert float(norm) == 0.0 and clipped == -1


# ---------------------------------------------------------------------------------------------------------- rigs --
def set_tau(rig, tau):
    L.check(rig.lib, rig.lib.rb_learner_set_target_tau(rig.ad.h, tau, rig.mem.stream))


def target(rig):
    rig.mem.sync()
    return S._dl(rig.mem, rig.ad.p_tg)


def restore(rig, base):
    ad = rig.ad
    for k, buf in (("p", ad.p_on), ("m", ad.adam_m), ("v", ad.adam_v), ("t", ad.p_tg)):
        S._store(buf, base[k])


CASES = (("scales", "bite", 3), ("zeros", "idle", 2 ** 32 + 3))


def forms_check(lib, Mem, monkeypatch, cases=CASES, taus=TAUS, name="dataeff"):
    """k_clip_adam by value and by device counter, flush, hosted by k_sample, k_adam_pending_ema behind a 25-transition window: every
    form from the SAME state (restored before every pass) with tau = 0 and with every tau."""
    n25 = name + "-n21"
    monkeypatch.setitem(scenarios.LEARN_CONFIGS, n25, dict(scenarios.LEARN_CONFIGS[name], multi_step=21))
    monkeypatch.setenv("RB_OPTS", "spec_draw=0")
    D = L.LEARNER_DEFER_UPDATE
    rigs = dict(value=S.build_rig(lib, Mem, name, False), device=S.build_rig(lib, Mem, name, False),
                flush=S.build_rig(lib, Mem, name, False, D), hosted=S.build_rig(lib, Mem, name, True, D),
                hosted25=S.build_rig(lib, Mem, n25, True, D))
    assert rigs["hosted25"].rp.bufs.window_len == 25 and rigs["hosted"].rp.bufs.window_len <= 24
    first = rigs["value"]
    layout, n = first.ad.layout, first.ad.n_params
    rs = np.random.RandomState(17)
    base = dict(p=S._dl(first.mem, first.ad.p_on), t=S._dl(first.mem, first.ad.p_tg), m=(1e-3 * rs.randn(n)).astype(F32),
                v=(1e-4 * rs.rand(n)).astype(F32))
    assert not np.array_equal(base["p"], base["t"])
    for ci, (pattern, kind, step) in enumerate(cases):
        g = S.make_grad(layout, n, 900 + ci, pattern)
        max_norm = S.resolve_max_norm(kind, g)
        targets = {}
        for fname, rig in rigs.items():
            form = {"hosted25": "hosted"}.get(fname, fname)
            restore(rig, base)
            set_tau(rig, 0.0)
            _, plain, pnorm, _ = S.run_synthetic(rig, form, g, max_norm, step)
            assert np.array_equal(_bits(target(rig)), _bits(base["t"])), (fname, "tau = 0 must leave the target alone")
            assert not np.array_equal(_bits(plain["p"]), _bits(base["p"]))
            for tau in taus:
                restore(rig, base)
                set_tau(rig, tau)
                before, after, norm, hosted = S.run_synthetic(rig, form, g, max_norm, step)
                label = "%s/%s/%s" % (fname, pattern, kind)
                if form == "hosted":
                    assert hosted == 1, label
                S.same_state(plain, after, (label, tau, "(i)"))
                assert _bits(norm) == _bits(pnorm), (label, tau, "norm")
                t1 = target(rig)
                check_target(fname, tau, base["t"], after["p"], t1, label)
                targets.setdefault(tau, {})[fname] = t1
        for tau, per_form in targets.items():
            for fname, t1 in per_form.items():
                assert np.array_equal(_bits(t1), _bits(per_form["value"])), ("(iv)", ci, tau, fname)
    for rig in rigs.values():
        S.close_rig(rig)


def pairs_check(lib, Mem, monkeypatch, taus=TAUS, name="dataeff", opts="implicit_small=1,spec_draw=0"):
    """Real train steps under DEFER_UPDATE | IMPLICIT_SIGMA leave the (mu, sigma) pair pass pending.  Rig `flush` runs it by
    rb_learner_flush (k_adam_pending_ema), rig `hosted` in the next sampler launch (k_sample<1024, 4, true>), rig `plain` by flush
    with tau = 0; after every round `plain` is handed the others' target so that all three see the same next step."""
    flags = L.LEARNER_DEFER_UPDATE | L.LEARNER_IMPLICIT_SIGMA
    monkeypatch.setenv("RB_OPTS", opts)
    assert S.plan_reports_implicit_sigma(lib, name, opts, flags), "the shape must take the implicit sigma gradient"
    rigs = dict(pairs_flush=S.build_rig(lib, Mem, name, True, flags), pairs_hosted=S.build_rig(lib, Mem, name, True, flags),
                plain=S.build_rig(lib, Mem, name, True, flags))
    B = scenarios.LEARN_CONFIGS[name]["batch"]
    for rnd, tau in enumerate(taus):
        max_norm = (10.0, 1e-3)[rnd % 2]
        res = {}
        for tag, rig in rigs.items():
            m, ad = rig.mem, rig.ad
            set_tau(rig, 0.0 if tag == "plain" else tau)
            ts = ts_args(name, m, rig.rp, ad, rig.out, rig.job, 0.4, 0, max_norm)
            ts.norm_dev = m.ptr(rig.norm)
            L.check(lib, lib.rb_learner_train_step(ad.h, C.byref(ts), m.stream))
            t0 = target(rig)                                      # (the pass is pending: the target has not moved yet)
            job2 = L.NoiseJob()
            L.check(lib, lib.rb_learner_noise_job(ad.h, 2, C.byref(job2)))
            if tag == "pairs_hosted":
                job_out = L.NoiseJob()
                assert lib.rb_learner_attach_pending(ad.h, C.byref(job2), B, C.byref(job_out)) == 1
                S._sample(rig, job_out)
                L.check(lib, lib.rb_learner_pending_launched(ad.h))
            else:
                L.check(lib, lib.rb_learner_flush(ad.h, m.stream))
                S._sample(rig, job2)                              # the twin sampler launch that hosts nothing
            mid = S.state(rig)
            L.check(lib, lib.rb_learner_flush(ad.h, m.stream))    # (materialises the sigma gradient where the pass stored none)
            end = S.state(rig)
            S.same_state(mid, end, (tag, "flush after the pass"), keys=("p", "m", "v"))
            norm = F32(S._dl(m, rig.norm)[0])
            assert (float(norm) > max_norm) == (max_norm < 1.0), (tag, max_norm, float(norm))
            res[tag] = (end, norm, t0, target(rig))
        assert np.array_equal(_bits(res["plain"][3]), _bits(res["plain"][2])), "tau = 0 must leave the target alone"
        for tag in ("pairs_flush", "pairs_hosted"):
            end, norm, t0, t1 = res[tag]
            S.same_state(res["plain"][0], end, (tag, tau, "(i)"))
            assert _bits(norm) == _bits(res["plain"][1]), (tag, tau, "norm")
            assert np.array_equal(_bits(t0), _bits(res["plain"][2]))
            check_target(tag, tau, t0, end["p"], t1, "%s/max_norm %g" % (tag, max_norm))
        assert np.array_equal(_bits(res["pairs_flush"][3]), _bits(res["pairs_hosted"][3])), ("(iv) pairs", tau)
        S._store(rigs["plain"].ad.p_tg, res["pairs_flush"][3])
    for rig in rigs.values():
        S.close_rig(rig)


def fused_tile_check(lib, Mem, taus=TAUS, name="dataeff"):
    """learn under FUSE_FC_H_DW | WRITE_FUSED_GRADS, then rb_learner_clip_adam: k_clip_adam<4, true, true> carries no EMA, the
    stand-alone k_target_ema follows it.  Twin with tau = 0, handed the other's target after every step."""
    flags = L.LEARNER_FUSE_FC_H_DW | L.LEARNER_WRITE_FUSED_GRADS
    rigs = dict(fused_tile=S.build_rig(lib, Mem, name, False, flags), plain=S.build_rig(lib, Mem, name, False, flags))
    c = scenarios.LEARN_CONFIGS[name]
    draws = O.noise_draw_count(O.Config(**c))
    rs = np.random.RandomState(21)
    for k, tau in enumerate(taus):
        step, max_norm = k + 1, (1e-3, 10.0)[k % 2]
        raw_on, raw_tg = rs.randn(draws).astype(F32), rs.randn(draws).astype(F32)
        batch = scenarios.make_batch(c, 40 + step)
        res = {}
        for tag, rig in rigs.items():
            set_tau(rig, 0.0 if tag == "plain" else tau)
            rig.ad.reset_noise_online(raw_on)
            rig.ad.learn_only(batch, raw_tg)
            t0 = target(rig)
            S._clip_adam(rig, lib.rb_learner_clip_adam, max_norm, step, rig.mem.ptr(rig.norm))
            res[tag] = (S.state(rig), F32(S._dl(rig.mem, rig.norm)[0]), t0, target(rig))
        end, norm, t0, t1 = res["fused_tile"]
        assert (float(norm) > max_norm) == (max_norm < 1.0)
        S.same_state(res["plain"][0], end, ("fused_tile", tau, "(i)"))
        assert _bits(norm) == _bits(res["plain"][1])
        assert np.array_equal(_bits(res["plain"][3]), _bits(t0)) and np.array_equal(_bits(res["plain"][2]), _bits(t0))
        check_target("fused_tile", tau, t0, end["p"], t1, "fused_tile/max_norm %g" % max_norm)
        S._store(rigs["plain"].ad.p_tg, t1)
    for rig in rigs.values():
        S.close_rig(rig)


def failed_draw_check(lib, Mem, flags, hows, name="dataeff"):
    """The batch behind the gradient was a failed draw (the 16-slot ring of optimizer_scenarios.skipped_update_check as the
    learner's priority sink): with tau = 0.5 and then 1 the target is bit-unchanged, like p, m, v, and the norm is 0.
    hows: 'hosted' / 'flush' (DEFER_UPDATE), 'value' (k_clip_adam; under FUSE_FC_H_DW the tile pass and k_target_ema behind it)."""
    rig = S.build_rig(lib, Mem, name, False, flags)
    m, ad = rig.mem, rig.ad
    c = scenarios.LEARN_CONFIGS[name]
    B = c["batch"]
    fused = bool(flags & L.LEARNER_FUSE_FC_H_DW)
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
    S._store(ad.adam_m, np.full(ad.n_params, 0.25, np.float32))      # an un-skipped pass WOULD move everything
    S._store(ad.adam_v, np.full(ad.n_params, 1e-4, np.float32))
    draws = O.noise_draw_count(O.Config(**c))
    g = S.make_grad(ad.layout, ad.n_params, 700, "scales")
    for how in hows:
        for tau in (0.5, 1.0):
            set_tau(rig, tau)
            ad.reset_noise_online(rs.randn(draws).astype(np.float32))
            batch = scenarios.make_batch(c, 17)
            batch["weights"] = np.zeros(B, np.float32)                     # what the sampler wrote
            ad.learn_only(batch, rs.randn(draws).astype(np.float32))       # its head kernel copies the failed status
            if not fused:
                S._store(ad.grads, g)
                L.check(lib, lib.rb_learner_grads_modified(ad.h))
            S._store(rig.norm, np.full(1, -1.0, np.float32))
            before, t0 = S.state(rig), target(rig)
            if how == "value":
                S._clip_adam(rig, lib.rb_learner_clip_adam, 1e-3, 1, m.ptr(rig.norm))
            else:
                S._clip_adam(rig, lib.rb_learner_clip_adam_deferred, 1e-3, 0, m.ptr(rig.norm))
                if how == "hosted":
                    job_out = L.NoiseJob()
                    assert lib.rb_learner_attach_pending(ad.h, C.byref(job), B, C.byref(job_out)) == 1
                    draw(job_out)
                    L.check(lib, lib.rb_learner_pending_launched(ad.h))
                else:
                    L.check(lib, lib.rb_learner_flush(ad.h, m.stream))
            S.same_state(before, S.state(rig), ("failed draw", how, tau), keys=("p", "m", "v"))
            assert np.array_equal(_bits(target(rig)), _bits(t0)), ("failed draw: the target moved", how, tau)
            assert float(S._dl(m, rig.norm)[0]) == 0.0, (how, "the skipped pass reports norm 0")
    L.check(lib, lib.rb_learner_set_priority_sink(ad.h, None, None))
    S.close_rig(rig)
    rp.close()
