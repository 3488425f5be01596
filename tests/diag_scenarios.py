"""Device-side diagnostics through the C ABI: the ring of per-step records (rb_learner_set_stats, csrc/learn_stats.h k_step_stats),
the held-out loss (rb_learner_eval_loss) and the priority statistics of a replay (rb_replay_priority_stats, csrc/replay_stats.h
k_priority_stats).  The bodies run on the host interpreter (test_diag_emu.py) and on the device (test_diag_gpu.py).

Shapes.  Net: BASE of head_shapes_scenarios.py (data-efficient, hidden 32, batch 5); (atoms, actions) = (2, 1), (51, 6), (65, 8),
(256, 4) — every ZI of the head; batch 33 (three row groups of k_step_stats: the ticket fold) at (51, 6) and (256, 4); on the device
also the canonical net, hidden 512, batch 32, whose list of norm partials is longer than the 256 threads that sum it.

A record is compared with a numpy float64 evaluation of rb_step_stats_t's definitions (include/rainbow_hip.h) on the DEVICE's own
buffers: log_ps_a and m (rb_learner_debug_read 0 / 1), loss_dev and the step's weights, returns and nonterminals.  Tolerances:
  loss_mean, wloss_mean, weight_mean, return_mean   rtol 1e-6    one f32 rounding (6e-8) of a double sum, 16x margin
  q_mean, q_target_mean, td_abs_mean                atol 1e-6 max(|v_min|, |v_max|)
  entropy_mean                                      atol 4e-6
    (an f32 expf is within 2 ulp = 2.4e-7 relative in p; sum |z| p <= V and sum p |log p| <= ln Z <= 5.6; 4x margin)
  step, batch, status, terminal_frac, loss_max      exact;   grad_norm   the bits of norm_dev
The observed errors are printed by every case ("diag record ...") and collected in profiles/diag_bounds.txt.

Held-out loss: O.forward with noise None (eval mode, both networks) and O.project, recomposed below; loss rtol 2e-5 atol 1e-6, m
rtol 1e-4 atol 1e-6.  Seeds: every a* of the float64 reference has a top-two gap of at least GAP_SHARE of the support's width
(asserted, "ill-conditioned seed"; no case skipped or masked).  The head table's seeds were chosen under noise; EVAL_SEEDS below
were re-chosen in eval mode (`PYTHONPATH=.:tests python tests/diag_scenarios.py seeds`: first seed from 1 with a factor 2.5 to spare)."""
import ctypes as C

import numpy as np

import head_oracle as HO
import scenarios
from cabi_adapter import CAbiLearnAdapter, CAbiReplayAdapter, NumpyMem
from guarded_mem import PoisonedNumpyMem, PoisonedTorchMem
from head_shapes_scenarios import BASE, GAP_SHARE
from oracle import learner_oracle as O
from rainbow_amd import _lib as L
from rainbow_amd.agent_stats import STEP_STATS_DTYPE

RB_ERR_INVALID, RB_ERR_STATE = -1, -4

# case id: (atoms, actions, overrides of BASE)
CASES = {
    "z2-a1": (2, 1, {}),
    "z51-a6": (51, 6, {}),
    "z65-a8": (65, 8, {}),
    "z256-a4": (256, 4, {}),
    "z51-a6-b33": (51, 6, dict(batch=33)),
    "z256-a4-b33": (256, 4, dict(batch=33)),
}
# the host interpreter takes ~25 s per batch-33 step pair: it runs one batch-33 case, on the eager path (the fold over three row
# groups), and again for rb_learner_eval_loss (forwards only: the three-group fold of the record path once more, at a third of the
# price), and the four shapes at batch 5 everywhere; the device runs every case on every path
EMU_CASES = ("z2-a1", "z51-a6", "z65-a8", "z256-a4")
EMU_B33_CASE = "z51-a6-b33"
GPU_ONLY_CASES = {"canon-b32": (51, 6, dict(architecture="canonical", hidden=512, batch=32))}
EVAL_SEEDS = {"z2-a1": 1, "z51-a6": 2, "z65-a8": 2, "z256-a4": 2, "z51-a6-b33": 4, "z256-a4-b33": 2, "canon-b32": 2}


def case_config(case):
    atoms, actions, over = dict(CASES, **GPU_ONLY_CASES)[case]
    return dict(BASE, atoms=atoms, actions=actions, **over)


def poisoned(mem):
    """The guarded, never-zeroed twin of a NumpyMem / TorchMem instance (tests/guarded_mem.py)."""
    return PoisonedNumpyMem() if isinstance(mem, NumpyMem) else PoisonedTorchMem()


def make_learner(lib, mem, case, c):
    name = "_diag_" + case
    scenarios.LEARN_CONFIGS[name] = c
    return CAbiLearnAdapter(lib, mem, name), name


def drop_config(name):
    scenarios.LEARN_CONFIGS.pop(name, None)


class Ring:
    """A record ring and its count word in caller-owned memory with guard bands; the ring is never zeroed (0xC5 bytes)."""

    def __init__(self, lib, mem, ad, capacity):
        self.lib, self.mem, self.ad, self.capacity = lib, mem, ad, capacity
        self.pm = poisoned(mem)
        self.ring = self.pm.empty((capacity * 64,), np.uint8)
        self.count = self.pm.upload(np.zeros(1, np.int64))
        L.check(lib, lib.rb_learner_set_stats(ad.h, self.pm.ptr(self.ring), capacity, self.pm.ptr(self.count)))

    def read(self):
        self.mem.sync()
        self.pm.sync()
        return int(self.pm.download(self.count)[0]), np.ascontiguousarray(self.pm.download(self.ring)).view(STEP_STATS_DTYPE).copy()

    def check_guards(self):
        n, bad = self.pm.check()
        assert not bad, "a record or the count was written outside its buffer: %s" % bad
        nb, nbad = C.c_int64(0), C.c_int64(0)
        L.check(self.lib, self.lib.rb_debug_check_guards(C.byref(nb), C.byref(nbad)))
        assert nbad.value == 0, "%d library allocations with a damaged guard band" % nbad.value

    def off(self):
        L.check(self.lib, self.lib.rb_learner_set_stats(self.ad.h, None, 0, None))


# =============================================================================== the reference of a record
def record_reference(c, log_ps_a, m, loss, weights, returns, nonterminals):
    """rb_step_stats_t's float fields in numpy float64, rounded to float32 once at the end."""
    f8 = lambda a: np.asarray(a, dtype=np.float64).reshape(-1)
    sup = HO.support32(O.Config(**c)).astype(np.float64)
    lp = np.asarray(log_ps_a, dtype=np.float64)
    p = np.exp(lp)
    q, qt = (p * sup).sum(1), (np.asarray(m, dtype=np.float64) * sup).sum(1)
    ent = -np.where(p > 0, p * lp, 0.0).sum(1)
    lo, w = f8(loss), f8(weights)
    B = lo.size
    return dict(loss_mean=lo.mean(), loss_max=np.float32(np.asarray(loss, dtype=np.float32).max()), wloss_mean=(w * lo).mean(),
                weight_mean=w.mean(), q_mean=q.mean(), q_target_mean=qt.mean(), td_abs_mean=np.abs(qt - q).mean(),
                entropy_mean=ent.mean(), return_mean=f8(returns).mean(),
                terminal_frac=np.float32(np.count_nonzero(f8(nonterminals) == 0) / B))


def assert_record(what, c, rec, ref, step, status, batch):
    V = max(abs(c["v_min"]), abs(c["v_max"]))
    assert int(rec["step"]) == step and int(rec["batch"]) == batch and int(rec["status"]) == status, \
        (what, int(rec["step"]), int(rec["batch"]), int(rec["status"]), (step, batch, status))
    assert np.float32(rec["terminal_frac"]) == np.float32(ref["terminal_frac"]), (what, rec["terminal_frac"], ref["terminal_frac"])
    assert np.float32(rec["loss_max"]) == np.float32(ref["loss_max"]), (what, rec["loss_max"], ref["loss_max"])
    assert np.float32(rec["reserved"]).view(np.uint32) == 0, what
    line = []
    for k in ("loss_mean", "wloss_mean", "weight_mean", "return_mean"):
        err = abs(float(rec[k]) - float(ref[k])) / max(abs(float(ref[k])), 1e-300)
        line.append("%s %.2e/1e-06" % (k, err))
    for k, tol in (("q_mean", 1e-6 * V), ("q_target_mean", 1e-6 * V), ("td_abs_mean", 1e-6 * V), ("entropy_mean", 4e-6)):
        line.append("%s %.2e/%.0e" % (k, abs(float(rec[k]) - float(ref[k])), tol))
    print("diag record %s: observed error / bound: %s" % (what, ", ".join(line)))
    for k in ("loss_mean", "wloss_mean", "weight_mean", "return_mean"):
        np.testing.assert_allclose(float(rec[k]), float(ref[k]), rtol=1e-6, atol=0, err_msg="%s %s" % (what, k))
    for k, tol in (("q_mean", 1e-6 * V), ("q_target_mean", 1e-6 * V), ("td_abs_mean", 1e-6 * V), ("entropy_mean", 4e-6)):
        np.testing.assert_allclose(float(rec[k]), float(ref[k]), rtol=0, atol=tol, err_msg="%s %s" % (what, k))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def learn_inputs(c, seed, steps=2):
    cfg = O.Config(**c)
    online, target = O.init_params(cfg, seed), O.init_params(cfg, seed + 1000)
    rs = np.random.RandomState(seed + 2000)
    draws = O.noise_draw_count(cfg)
    per_step = [dict(raw_on=rs.randn(draws).astype(np.float32), raw_tg=rs.randn(draws).astype(np.float32),
                     batch=scenarios.make_batch(c, seed + 3000 + k)) for k in range(steps)]
    return cfg, online, target, per_step


# =============================================================================== A: step records, eager path
def check_records_eager(lib, mem, case):
    """Two learn steps as rb_learner_learn + rb_learner_clip_adam (step number from the device counter): each record against the
    float64 reference on the device's buffers, grad_norm the bits of norm_dev, ring and count inside their guard bands."""
    c = case_config(case)
    B, Z = c["batch"], c["atoms"]
    _cfg, online, target, steps = learn_inputs(c, 11)
    ad, name = make_learner(lib, mem, case, c)
    try:
        ad.step_from_device = True
        ad.load(online, target)
        ctr = mem.upload(np.zeros(1, np.int64))
        L.check(lib, lib.rb_learner_set_step_counter(ad.h, mem.ptr(ctr)))
        ring = Ring(lib, mem, ad, 4)
        for k, st in enumerate(steps):
            ad.reset_noise_online(st["raw_on"])
            ad.learn_only(st["batch"], st["raw_tg"])
            count, recs = ring.read()
            assert count == k + 1, (case, k, count)
            log_ps_a, m = ad.debug(0, (B, Z), np.float32), ad.debug(1, (B, Z), np.float32)
            out = ad.finish_step()
            b = st["batch"]
            ref = record_reference(c, log_ps_a, m, out["loss"], b["weights"], b["returns"], b["nonterminals"])
            assert_record("%s eager step %d" % (case, k), c, recs[k], ref, k + 1, 0, B)
            assert np.float32(recs[k]["grad_norm"]).view(np.uint32) == np.float32(out["grad_norm"]).view(np.uint32), \
                (case, k, float(recs[k]["grad_norm"]), out["grad_norm"])
            assert float(out["grad_norm"]) > 0
        ring.check_guards()
        ring.off()
    finally:
        ad.close()
        drop_config(name)


# =============================================================================== the one-call path (rb_learner_train_step)
def ts_build(lib, mem, c, name, capacity=512, appends=600, flags=0, seed=5):
    """ts_scenarios.ts_build for a configuration of this file and a Mem INSTANCE: a filled replay, a learner with a priority sink
    into it, a device step counter, and the buffers of one rb_learner_train_step call."""
    B, h, n = c["batch"], c["history"], c["multi_step"]
    scenarios.LEARN_CONFIGS[name] = c
    rp = CAbiReplayAdapter(lib, mem, capacity, h, n, c["discount"], 0.5)
    rs = np.random.RandomState(seed)
    for _ in range(appends):
        rp.append(scenarios.synth_state(rs, h, 0), int(rs.randint(0, c["actions"])), float(rs.choice([-1.0, 0.0, 1.0])),
                  bool(rs.random_sample() < 0.05))
    ad = CAbiLearnAdapter(lib, mem, name)
    ad.learner_flags = flags
    cfg = O.Config(**c)
    ad.load(O.init_params(cfg, 1), O.init_params(cfg, 2))
    ad.reset_noise_online(rs.randn(O.noise_draw_count(cfg)).astype(np.float32))
    out = dict(tree_idx=mem.empty((B,), np.int64), actions=mem.empty((B,), np.int64), returns=mem.empty((B,), np.float32),
               nonterm=mem.empty((B,), np.float32), weights=mem.empty((B,), np.float32), loss=mem.empty((B,), np.float32),
               norm=mem.empty((1,), np.float32), ctr=mem.upload(np.zeros(1, np.int64)))
    L.check(lib, lib.rb_learner_set_priority_sink(ad.h, rp.h, mem.ptr(out["tree_idx"])))
    L.check(lib, lib.rb_learner_set_step_counter(ad.h, mem.ptr(out["ctr"])))
    job = L.NoiseJob()
    L.check(lib, lib.rb_learner_noise_job(ad.h, 1, C.byref(job)))
    return rp, ad, out, job


def ts_call(lib, mem, c, rp, ad, o, job, beta=0.4):
    hy = scenarios.LEARN_HYPER
    ts = L.TrainStep(replay=rp.h, batch=c["batch"], max_attempts=64, window_len=rp.bufs.window_len, priority_weight=beta,
                     tree_idx_dev=mem.ptr(o["tree_idx"]), actions_dev=mem.ptr(o["actions"]), returns_dev=mem.ptr(o["returns"]),
                     nonterminals_dev=mem.ptr(o["nonterm"]), weights_dev=mem.ptr(o["weights"]), noise_job=C.addressof(job),
                     frames_dev=rp.bufs.frames_dev, windows_dev=rp.bufs.window_dev, loss_dev=mem.ptr(o["loss"]),
                     exp_avg_dev=mem.ptr(ad.adam_m), exp_avg_sq_dev=mem.ptr(ad.adam_v), norm_dev=mem.ptr(o["norm"]), lr=hy["lr"],
                     beta1=0.9, beta2=0.999, eps=hy["adam_eps"], step=0, max_norm=hy["norm_clip"])
    L.check(lib, lib.rb_learner_train_step(ad.h, C.byref(ts), mem.stream))


def ts_state(mem, rp, ad, o):
    mem.sync()
    return dict(idx=mem.download(o["tree_idx"]).copy(), loss=mem.download(o["loss"]).copy(), w=mem.download(o["weights"]).copy(),
                params=mem.download(ad.p_on).copy(), target=mem.download(ad.p_tg).copy(), m=mem.download(ad.adam_m).copy(),
                v=mem.download(ad.adam_v).copy(), noise_on=mem.download(ad.z_on).copy(), noise_tg=mem.download(ad.z_tg).copy(),
                tree=rp.tree().copy(), norm=mem.download(o["norm"]).copy(), grads=mem.download(ad.grads).copy(),
                ctr=mem.download(o["ctr"]).copy())


def check_records_one_call(lib, mem, case, flags=L.LEARNER_DEFER_UPDATE):
    """Two rb_learner_train_step calls with the optimiser pass left pending (RB_LEARNER_DEFER_UPDATE): each record against the
    reference on the device's buffers; grad_norm the bits of what the pass writes to norm_dev once rb_learner_flush has run it."""
    c = case_config(case)
    B, Z = c["batch"], c["atoms"]
    name = "_diag_ts_" + case
    rp, ad, o, job = ts_build(lib, mem, c, name, flags=flags)
    try:
        ring = Ring(lib, mem, ad, 4)
        for k in range(2):
            ts_call(lib, mem, c, rp, ad, o, job)
            count, recs = ring.read()
            assert count == k + 1
            log_ps_a, m = ad.debug(0, (B, Z), np.float32), ad.debug(1, (B, Z), np.float32)     # (runs the pending pass first)
            L.check(lib, lib.rb_learner_flush(ad.h, mem.stream))
            mem.sync()
            dl = mem.download
            ref = record_reference(c, log_ps_a, m, dl(o["loss"]), dl(o["weights"]), dl(o["returns"]), dl(o["nonterm"]))
            assert_record("%s one-call step %d" % (case, k), c, recs[k], ref, k + 1, 0, B)
            norm = np.float32(dl(o["norm"])[0])
            assert np.float32(recs[k]["grad_norm"]).view(np.uint32) == norm.view(np.uint32), (case, k, float(recs[k]["grad_norm"]), float(norm))
            assert float(norm) > 0 and int(dl(o["ctr"])[0]) == k + 1
        ring.check_guards()
        ring.off()
    finally:
        ad.close(); rp.close()
        drop_config(name)


def check_ring_wraps(lib, mem):
    """Capacity 3 and five steps: count 5, the slots hold steps 3, 4, 5 in ring order (record i in slot i % 3); what a reader that
    last read at count 0 has lost is 2 records."""
    case = "z51-a6"
    c = case_config(case)
    name = "_diag_wrap"
    rp, ad, o, job = ts_build(lib, mem, c, name)
    try:
        ring = Ring(lib, mem, ad, 3)
        for _ in range(5):
            ts_call(lib, mem, c, rp, ad, o, job)
        count, recs = ring.read()
        assert count == 5
        assert [int(r["step"]) for r in recs] == [4, 5, 3], [int(r["step"]) for r in recs]      # slots 0, 1, 2 = records 3, 4, 2
        order = [recs[i % 3] for i in range(count - 3, count)]
        assert [int(r["step"]) for r in order] == [3, 4, 5]
        assert count - 3 - 0 == 2                                                                  # dropped, for a first read
        assert all(int(r["batch"]) == c["batch"] and int(r["status"]) == 0 and np.isfinite(r["loss_mean"]) for r in recs)
        ring.check_guards()
    finally:
        ad.close(); rp.close()
        drop_config(name)


def check_failed_draw(lib, mem):
    """A replay too small for the batch (scenarios.sampler_gives_up_check's ring: 16 slots, batch 8): the step's record has
    status != 0, zero weights, and the step counter — preset to 7 — has not advanced."""
    c = dict(case_config("z51-a6"), batch=8)
    name = "_diag_fail"
    rp, ad, o, job = ts_build(lib, mem, c, name, capacity=16, appends=16)
    try:
        if isinstance(o["ctr"], np.ndarray):
            o["ctr"][0] = 7
        else:
            o["ctr"].fill_(7)
        ring = Ring(lib, mem, ad, 2)
        ts_call(lib, mem, c, rp, ad, o, job)
        count, recs = ring.read()
        assert rp.raw_header().last_status != 0, "the scenario needs a draw that gives up"
        assert count == 1 and int(recs[0]["status"]) != 0 and int(recs[0]["step"]) == 7 and int(recs[0]["batch"]) == 8
        assert float(recs[0]["weight_mean"]) == 0.0 and float(recs[0]["wloss_mean"]) == 0.0
        assert int(mem.download(o["ctr"])[0]) == 7
        L.check(lib, lib.rb_replay_reset_failed_samples(rp.h))
        ring.check_guards()
    finally:
        ad.close(); rp.close()
        drop_config(name)


def check_exchange_gives_nan(lib, mem):
    """With the replica exchange armed (world 2, the setup of exchange_scenarios.check_learn) the gradient is complete only after
    rb_learner_finish_grads: grad_norm is NaN, everything else is the record of the step.  rb_learner_eval_loss refuses while the
    gradients wait for it, and works again afterwards."""
    import exchange_scenarios as XS
    case = "z51-a6"
    c = case_config(case)
    B, Z = c["batch"], c["atoms"]
    _cfg, online, target, steps = learn_inputs(c, 11, steps=1)
    ad, name = make_learner(lib, mem, "xch", c)
    try:
        ad.load(online, target)
        stride = XS.exchange_layout(lib, ad)[0]
        lo, al = mem.upload(np.zeros(stride, dtype=np.float32)), mem.empty((2 * stride,), np.float32)
        L.check(lib, lib.rb_learner_set_exchange(ad.h, 2, mem.ptr(lo), mem.ptr(al)))
        ring = Ring(lib, mem, ad, 2)
        st = steps[0]
        ad.reset_noise_online(st["raw_on"])
        ad.learn_only(st["batch"], st["raw_tg"])
        count, recs = ring.read()
        assert count == 1 and np.isnan(recs[0]["grad_norm"]), recs[0]
        b = st["batch"]
        ref = record_reference(c, ad.debug(0, (B, Z), np.float32), ad.debug(1, (B, Z), np.float32), mem.download(ad._loss),
                               b["weights"], b["returns"], b["nonterminals"])
        assert_record("%s exchange" % case, c, recs[0], ref, -1, 0, B)
        # ---- the held-out loss refuses while the factors wait for the exchange
        bufs, loss = ad._bufs, mem.empty((B,), np.float32)
        args = (ad.h, mem.ptr(bufs["states"]), mem.ptr(bufs["next_states"]), mem.ptr(bufs["actions"]), mem.ptr(bufs["returns"]),
                mem.ptr(bufs["nonterminals"]), mem.ptr(loss), None, mem.stream)
        assert lib.rb_learner_eval_loss(*args) == RB_ERR_STATE
        assert b"rb_learner_finish_grads" in lib.rb_last_error()
        XS.fill(al, np.concatenate([mem.download(lo), mem.download(lo)]))
        L.check(lib, lib.rb_learner_finish_grads(ad.h, mem.stream))
        L.check(lib, lib.rb_learner_eval_loss(*args))
        mem.sync()
        assert np.isfinite(mem.download(loss)).all()
        ring.off()
    finally:
        lib.rb_learner_set_exchange(ad.h, 1, None, None)
        ad.close()
        drop_config(name)


def check_deterministic_and_off(lib, mem, count_launches, case="z51-a6-b33", steps=2):
    """Three identical handles run the same two steps: with a ring, never with one, and with a ring set and taken away again.
    The two ringed steps of handle 0 repeated on a fourth, identical handle give bit-identical records; all parameters, moments,
    gradients and trees are bit-identical; on the device (count_launches) a ringed step issues exactly one launch more, and that
    launch is k_step_stats.  (The host interpreter runs workgroups one after the other: there a small batch and one step do.)"""
    c = case_config(case)
    hs = [ts_build(lib, mem, c, "_diag_off%d" % i) for i in range(4)]
    try:
        rings = [Ring(lib, mem, hs[0][1], 4), None, Ring(lib, mem, hs[2][1], 4), Ring(lib, mem, hs[3][1], 4)]
        rings[2].off()
        launches = []
        for i, (rp, ad, o, job) in enumerate(hs):
            per = []
            for pat in ((b"k_", b"k_step_stats") if count_launches else (None,) * steps):
                if pat:
                    mem.sync()
                    L.check(lib, lib.rb_profile_select(pat))
                ts_call(lib, mem, c, rp, ad, o, job)
                if pat:
                    mem.sync()
                    n = C.c_int64(0)
                    L.check(lib, lib.rb_profile_read(None, C.byref(n)))
                    L.check(lib, lib.rb_profile_select(None))
                    per.append(int(n.value))
            launches.append(per)
        states = [ts_state(mem, rp, ad, o) for rp, ad, o, job in hs]
        for i in (1, 2, 3):
            for k in states[0]:
                assert same_bits(states[0][k], states[i][k]), ("handle %d" % i, k)
        (n0, r0), (n3, r3) = rings[0].read(), rings[3].read()
        assert n0 == n3 == steps and same_bits(r0[:steps], r3[:steps]), (r0[:steps], r3[:steps])
        assert rings[2].read()[0] == 0
        if count_launches:
            print("diag launches per step (all, k_step_stats): ring %s, never set %s, set then cleared %s" % tuple(launches[:3]))
            assert launches[0][1] == 1 and launches[1][1] == 0 and launches[2][1] == 0
            assert launches[0][0] == launches[1][0] + 1 == launches[2][0] + 1, launches
        for r in (rings[0], rings[2], rings[3]):
            r.check_guards()
    finally:
        for i, (rp, ad, o, job) in enumerate(hs):
            ad.close(); rp.close()
            drop_config("_diag_off%d" % i)


# =============================================================================== B: the held-out loss
def heldout_reference(c, online, target, batch):
    """Agent.learn's loss with both networks in eval mode and no gradient: O.forward (noise None) and O.project, recomposed.
    Returns (loss, m, min top-two gap of the float64 expected values of online(next_states))."""
    import torch
    cfg = O.Config(**c)
    B = c["batch"]
    with torch.no_grad():
        p_on = {k: torch.as_tensor(np.ascontiguousarray(v)) for k, v in online.items()}
        p_tg = {k: torch.as_tensor(np.ascontiguousarray(v)) for k, v in target.items()}
        states = torch.as_tensor(batch["states"]).to(torch.float32).div(255)
        next_states = torch.as_tensor(batch["next_states"]).to(torch.float32).div(255)
        actions = torch.as_tensor(batch["actions"]).to(torch.int64)
        log_ps_a = O.forward(cfg, p_on, None, states, log=True)[torch.arange(B), actions]
        pns = O.forward(cfg, p_on, None, next_states)
        ev = (pns.numpy().astype(np.float64) * HO.support32(cfg).astype(np.float64)).sum(axis=2)
        a_star = torch.as_tensor(ev.argmax(axis=1))
        pns_a = O.forward(cfg, p_tg, None, next_states)[torch.arange(B), a_star]
        m, _l, _u, _b = O.project(cfg, pns_a, torch.as_tensor(batch["returns"]).to(torch.float32),
                                  torch.as_tensor(batch["nonterminals"]).to(torch.float32).reshape(B))
        loss = -torch.sum(m * log_ps_a, 1)
    return loss.numpy(), m.numpy(), float(HO.top2_gap(ev).min()), a_star.numpy()


def eval_inputs(case):
    c = case_config(case)
    seed = EVAL_SEEDS[case]
    cfg = O.Config(**c)
    return c, O.init_params(cfg, seed), O.init_params(cfg, seed + 1000), scenarios.make_batch(c, seed + 3000)


def upload_batch(mem, c, batch):
    B = c["batch"]
    return dict(states=mem.upload(batch["states"]), next_states=mem.upload(batch["next_states"]),
                actions=mem.upload(batch["actions"].astype(np.int64)), returns=mem.upload(batch["returns"]),
                nonterminals=mem.upload(batch["nonterminals"].astype(np.float32).reshape(B)))


def eval_loss(lib, mem, ad, bufs, loss, rec=None):
    L.check(lib, lib.rb_learner_eval_loss(ad.h, mem.ptr(bufs["states"]), mem.ptr(bufs["next_states"]), mem.ptr(bufs["actions"]),
                                          mem.ptr(bufs["returns"]), mem.ptr(bufs["nonterminals"]), mem.ptr(loss),
                                          mem.ptr(rec) if rec is not None else None, mem.stream))
    mem.sync()


def check_eval_loss(lib, mem, case):
    """rb_learner_eval_loss against the recomposed oracle; the online AND the target noise are set to non-zero draws first, so a
    forward of either network that read its noise buffer would miss.  Its record (a poisoned, guarded 64-byte buffer) against the float64 reference on the device's buffers, with
    step -1, unit weights and grad_norm NaN; twice gives the same bits."""
    c, online, target, batch = eval_inputs(case)
    B, Z = c["batch"], c["atoms"]
    want_loss, want_m, gap, want_a = heldout_reference(c, online, target, batch)
    width = c["v_max"] - c["v_min"]
    print("diag eval_loss %s seed %d: min a* gap %.3e" % (case, EVAL_SEEDS[case], gap))
    assert gap >= GAP_SHARE * width, "ill-conditioned seed: a* top-two gap %.3e" % gap
    ad, name = make_learner(lib, mem, "ev-" + case, c)
    try:
        ad.load(online, target)
        rs3, draws = np.random.RandomState(3), O.noise_draw_count(O.Config(**c))
        ad.reset_noise_online(rs3.randn(draws).astype(np.float32))
        raw_tg = mem.upload(rs3.randn(draws).astype(np.float32))          # ... and the target's: eval mode must ignore both buffers
        L.check(lib, lib.rb_learner_reset_noise(ad.h, 1, mem.ptr(raw_tg), mem.stream))
        mem.sync()
        assert np.abs(mem.download(ad.z_on)).max() > 0 and np.abs(mem.download(ad.z_tg)).max() > 0
        bufs = upload_batch(mem, c, batch)
        pm = poisoned(mem)
        loss, rec = pm.empty((B,), np.float32), pm.empty((64,), np.uint8)
        eval_loss(lib, mem, ad, bufs, loss, rec)
        pm.sync()
        got_loss = pm.download(loss).copy()
        r = np.ascontiguousarray(pm.download(rec)).view(STEP_STATS_DTYPE).copy()[0]
        assert np.array_equal(ad.debug(2, (B,), np.int32).astype(np.int64), want_a)
        log_ps_a, m = ad.debug(0, (B, Z), np.float32), ad.debug(1, (B, Z), np.float32)
        np.testing.assert_allclose(m, want_m, rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(got_loss, want_loss, rtol=2e-5, atol=1e-6)
        ref = record_reference(c, log_ps_a, m, got_loss, np.ones(B, np.float32), batch["returns"], batch["nonterminals"])
        assert_record("%s eval_loss" % case, c, r, ref, -1, 0, B)
        assert np.isnan(r["grad_norm"]) and float(r["weight_mean"]) == 1.0
        eval_loss(lib, mem, ad, bufs, loss, rec)
        pm.sync()
        assert same_bits(pm.download(loss), got_loss) and same_bits(pm.download(rec), np.frombuffer(r.tobytes(), np.uint8))
        assert not pm.check()[1], pm.check()[1]
        # loss alone: no record asked for
        eval_loss(lib, mem, ad, bufs, loss, None)
        assert same_bits(pm.download(loss), got_loss)
    finally:
        ad.close()
        drop_config(name)


def check_eval_no_side_effects(lib, mem):
    """Twins run train_step; one of them evaluates a held-out batch in between.  Around the call (after rb_learner_flush, so that the
    pending pass it would run first has run) every buffer it must leave alone is bit-identical — parameters, target, moments,
    gradients, both noise buffers, the noise epoch, the step counter, the norm, the sink's tree; and the next step equals the twin's."""
    case = "z51-a6"
    c = case_config(case)
    hs = [ts_build(lib, mem, c, "_diag_se%d" % i, flags=L.LEARNER_DEFER_UPDATE) for i in range(2)]
    try:
        def rng(ad):
            s, e = C.c_uint64(0), C.c_uint64(0)
            L.check(lib, lib.rb_learner_get_rng(ad.h, C.byref(s), C.byref(e), mem.stream))
            return s.value, e.value
        for rp, ad, o, job in hs:
            ts_call(lib, mem, c, rp, ad, o, job)
        rp, ad, o, job = hs[0]
        L.check(lib, lib.rb_learner_flush(ad.h, mem.stream))
        before, rng_before = ts_state(mem, rp, ad, o), rng(ad)
        bufs = upload_batch(mem, c, scenarios.make_batch(c, 99))
        loss = mem.empty((c["batch"],), np.float32)
        rec = mem.empty((64,), np.uint8)
        eval_loss(lib, mem, ad, bufs, loss, rec)
        after, rng_after = ts_state(mem, rp, ad, o), rng(ad)
        assert rng_before == rng_after
        for k in before:
            assert same_bits(before[k], after[k]), "rb_learner_eval_loss changed %s" % k
        assert np.isfinite(mem.download(loss)).all()
        for rp, ad, o, job in hs:
            ts_call(lib, mem, c, rp, ad, o, job)
        for rp, ad, o, job in hs:
            L.check(lib, lib.rb_learner_flush(ad.h, mem.stream))
        a, b = ts_state(mem, *hs[0][:3]), ts_state(mem, *hs[1][:3])
        for k in a:
            assert same_bits(a[k], b[k]), "the step after rb_learner_eval_loss differs from the twin's in %s" % k
        assert rng(hs[0][1]) == rng(hs[1][1])
    finally:
        for i, (rp, ad, o, job) in enumerate(hs):
            ad.close(); rp.close()
            drop_config("_diag_se%d" % i)


def check_eval_refusals(lib, mem):
    """Every NULL argument is refused with a message that names it."""
    c, online, target, batch = eval_inputs("z2-a1")
    ad, name = make_learner(lib, mem, "ev-null", c)
    try:
        ad.load(online, target)
        bufs = upload_batch(mem, c, batch)
        loss = mem.empty((c["batch"],), np.float32)
        full = [ad.h, mem.ptr(bufs["states"]), mem.ptr(bufs["next_states"]), mem.ptr(bufs["actions"]), mem.ptr(bufs["returns"]),
                mem.ptr(bufs["nonterminals"]), mem.ptr(loss), None, mem.stream]
        for i, arg in enumerate(["l", "states_dev", "next_states_dev", "actions_dev", "returns_dev", "nonterminals_dev", "loss_dev"]):
            a = list(full)
            a[i] = None
            assert lib.rb_learner_eval_loss(*a) == RB_ERR_INVALID, arg
            assert arg.encode() in lib.rb_last_error(), (arg, lib.rb_last_error())
        assert lib.rb_learner_set_stats(ad.h, mem.ptr(loss), 4, None) == RB_ERR_INVALID
        assert lib.rb_learner_set_stats(ad.h, mem.ptr(loss), 0, mem.ptr(loss)) == RB_ERR_INVALID
        assert lib.rb_learner_set_stats(None, None, 0, None) == RB_ERR_INVALID
        L.check(lib, lib.rb_learner_eval_loss(*full))
        mem.sync()
    finally:
        ad.close()
        drop_config(name)


# =============================================================================== C: priority statistics
PSTATS_STATES = ("empty", "partly-filled", "updated", "wide", "invalid")
# 64: one workgroup, most of its lanes beyond the leaves; 4098: one leaf pair beyond the 4096-leaf chunk of the first workgroup (the
# smallest capacity with a second one: rb_replay_create refuses odd capacities, so 4097 does not exist); 2^20, device only: 256 chunks
PSTATS_CAPACITIES = [64, 4098]


def pstats_reference(leaves):
    leaves = np.asarray(leaves, dtype=np.float32)
    bad = ~np.isfinite(leaves) | (leaves < 0)
    v = leaves[~bad & (leaves > 0)]
    hist = np.zeros(64, np.int64)
    if v.size:
        _m, e = np.frexp(v.astype(np.float64))                 # v = m 2^e with m in [0.5, 1): floor(log2 v) = e - 1
        k = np.where(v < np.float32(2.0 ** -126), 0, np.clip(e - 1 + 40, 0, 63))
        np.add.at(hist, k, 1)
    v8 = v.astype(np.float64)
    return dict(nonzero=int(v.size), invalid=int(bad.sum()), sum=float(v8.sum()), sumsq=float((v8 * v8).sum()),
                max=np.float32(v.max()) if v.size else np.float32(0), min_pos=np.float32(v.min()) if v.size else np.float32(0), hist=hist)


def pstats_run(lib, mem, rp):
    pm = poisoned(mem)
    out = pm.empty((C.sizeof(L.PriorityStats),), np.uint8)
    L.check(lib, lib.rb_replay_priority_stats(rp.h, pm.ptr(out), mem.stream))
    mem.sync(); pm.sync()
    raw = np.ascontiguousarray(pm.download(out)).tobytes()
    assert not pm.check()[1], pm.check()[1]
    return raw, L.PriorityStats.from_buffer_copy(raw)


def check_priority_stats(lib, mem, capacity, state):
    """rb_replay_priority_stats against numpy on the leaves copied back: counts, max, min_pos and the histogram exact, sum and
    sumsq within 1e-9 (double accumulation of at most 2^20 non-negative terms: n 2^-53 ~ 1e-10), the same bytes when repeated, and
    the whole struct overwritten (it starts as 0xC5 bytes)."""
    rp = CAbiReplayAdapter(lib, mem, capacity, 4, 3, 0.99, 0.5)
    try:
        ts = rp.bufs.tree_start
        rs = np.random.RandomState(capacity % 1000 + len(state))
        leaf = lambda slots: np.asarray(slots, dtype=np.int64) + ts
        if state != "empty":
            for _ in range(min(capacity - 8, 40)):                      # real appends: new transitions enter at the running maximum
                rp.append(scenarios.synth_state(rs, 4, 0), 1, 0.0, bool(rs.random_sample() < 0.1))
        if state in ("updated", "wide", "invalid"):
            n = min(capacity, 1024)
            # distinct slots, the last leaf and the first among them
            slots = np.concatenate([[capacity - 1, 0], 1 + rs.choice(capacity - 2, size=n - 2, replace=False)])
            if state == "updated":
                rp.update_leaves(leaf(slots), rs.uniform(0.01, 3.0, size=n).astype(np.float32))
            else:
                # more than 64 octaves, beyond both ends of the histogram, a denormal, the largest and the smallest normal
                vals = np.exp2(rs.uniform(-60, 40, size=n)).astype(np.float32)
                vals[:6] = [np.float32(2.0 ** -130), np.float32(2.0 ** -126), np.float32(2.0 ** -41), np.float32(2.0 ** -39),
                            np.float32(2.0 ** 23), np.float32(2.0 ** 24)]
                if state == "invalid":
                    vals[6], vals[7], vals[8] = np.float32("nan"), np.float32(-1.5), np.float32("inf")
                rp.update_leaves(leaf(slots), vals)
        leaves = rp.tree()[ts:ts + capacity]
        want = pstats_reference(leaves)
        raw, got = pstats_run(lib, mem, rp)
        what = "capacity %d %s" % (capacity, state)
        assert (got.nonzero, got.invalid) == (want["nonzero"], want["invalid"]), (what, got.nonzero, got.invalid, want["nonzero"], want["invalid"])
        assert np.float32(got.max) == want["max"] and np.float32(got.min_pos) == want["min_pos"], (what, got.max, got.min_pos, want["max"], want["min_pos"])
        assert np.array_equal(np.array(got.hist, dtype=np.int64), want["hist"]), (what, list(got.hist), want["hist"].tolist())
        np.testing.assert_allclose(got.sum, want["sum"], rtol=1e-9, atol=0, err_msg=what)
        np.testing.assert_allclose(got.sumsq, want["sumsq"], rtol=1e-9, atol=0, err_msg=what)
        if state == "empty":
            assert (got.nonzero, got.invalid, got.sum, got.sumsq, got.max, got.min_pos) == (0, 0, 0.0, 0.0, 0.0, 0.0) and not any(got.hist)
        if state in ("wide", "invalid"):
            assert got.hist[0] >= 3 and got.hist[1] >= 1 and got.hist[63] >= 2 and got.max / got.min_pos > 2.0 ** 64, what
        if state == "invalid":
            assert got.invalid == 3
        raw2, _ = pstats_run(lib, mem, rp)
        assert raw == raw2, "%s: the result changed when repeated" % what
        assert np.array_equal(rp.tree()[ts:ts + capacity].view(np.uint32), leaves.view(np.uint32)), "%s: the tree was written" % what
    finally:
        rp.close()


def check_priority_stats_refusals(lib, mem):
    rp = CAbiReplayAdapter(lib, mem, 64, 4, 3, 0.99, 0.5)
    try:
        out = mem.empty((C.sizeof(L.PriorityStats),), np.uint8)
        assert lib.rb_replay_priority_stats(None, mem.ptr(out), mem.stream) == RB_ERR_INVALID
        assert lib.rb_replay_priority_stats(rp.h, None, mem.stream) == RB_ERR_INVALID and b"out_dev" in lib.rb_last_error()
    finally:
        rp.close()


# =============================================================================== seed search (CPU, oracle only)
def find_seed(case, spare=2.5):
    c = case_config(case)
    cfg = O.Config(**c)
    width = c["v_max"] - c["v_min"]
    for seed in range(1, 200):
        batch = scenarios.make_batch(c, seed + 3000)
        gap = heldout_reference(c, O.init_params(cfg, seed), O.init_params(cfg, seed + 1000), batch)[2]
        if gap >= spare * GAP_SHARE * width:
            return seed, gap
    raise AssertionError("no seed below 200 for " + case)


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["seeds"]:
        for case in list(CASES) + list(GPU_ONLY_CASES):
            print(case, "seed %d: a* gap %.3e" % find_seed(case))
