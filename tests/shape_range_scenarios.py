"""The learn step and the act path over the accepted history ([1, 16]) and hidden ([1, 8192]) ranges: one learn body and one act
body, run on the host interpreter (test_shape_range_emu.py, the rows at batch 4) and on the device (test_shape_range_gpu.py, every
row) through the C ABI.  Every row of the table is the smallest shape on its side of a point where csrc/learner_plan.h or
csrc/act_host.h switches kernels, grids or buffers; tests/test_launch_plan.py pins, per row, the plan fields the row claims.

Every row: 51 atoms, 6 actions, multi_step 3, discount 0.99, support [-10, 10], batch 4, history 4, hidden 64 (canonical, "c-")
or 32 (data-efficient, "d-") unless its id says otherwise.

  case            crosses                                                                                    seed  ReLU margin, step 0 / 1
  c-hist1         split-K first layer k_conv_fwd_lds<GeomC1>, K 64 of the 256 staged; dW tile of 65 columns     1  5.8e-05 / 1.2e-05
  c-hist2         the same at K 128                                                                             0  1.1e-05 / 2.0e-06
  d-hist1         k_conv_fwd_lds<GeomD1> at K 25 of the 100 staged; dW tile of 26 columns                       0  5.4e-04 / 7.8e-06
  d-hist3         the same at K 75                                                                              2  5.4e-05 / 2.4e-04
  c-hist8         fast_conv 0: every conv on k_gemm, k_block_copy, k_dfeat_finish; act rows per workgroup 4     1  5.2e-06 / 4.6e-06
  c-hist16        the same at K = RB_ACT_KMAX (s_w and wreg[4] full); act rows per workgroup 1                  0  6.9e-05 / 2.8e-05
  d-hist16        fast_conv 0 at K 400; act rows per workgroup 2                                                0  1.5e-04 / 3.5e-05
  d-h1            generic FC (k_gemm); act_forward_single refuses (H & 3): the training forward acts            0  3.9e-02 / 1.6e-02
  d-h3            the same                                                                                      0  8.1e-03 / 2.8e-04
  d-h128          hsplits 1, the last                                                                           1  1.8e-04 / 1.2e-04
  d-h160          hsplits 2: the lazy dfeat sum with two partials                                               1  1.3e-04 / 5.0e-05
  d-h288          hsplits 3, equal splits of 192 rows                                                           4  2.4e-05 / 4.8e-06
  d-h352          hsplits 3, splits of 240 / 240 / 224 rows: a short last split                                 1  1.1e-04 / 3.5e-05
  d-h4096         the last fast_fc shape: the output layer's K = RB_NL_FWD_KMAX, s_ein full                     2  2.6e-06 / 3.1e-07
  d-h4128         the first generic shape above it: k_gemm everywhere, 52 row splits, k_dfeat_finish            3  1.3e-06 / 4.7e-06
  d-h8192         the accepted maximum (54 row splits)                                                          0  7.6e-07 / 5.2e-06
  c-b33-h2176     batch 33: the last hidden size with fuse_norm 1 (16 227 sum-of-squares slots of 16 384)       0  7.7e-08 / 3.4e-07
  c-b33-h2208     batch 33: fuse_norm 0 — streamed backward with sq_part = nullptr, norm from k_sumsq           5  1.1e-07 / 5.0e-07
  d-b1024-h4096   batch 1024: k_fc_gemm_fwd with 1536 tiles, above the 1024 that force split-K S = 1            2  1.2e-08 / 1.9e-08   masked

A correction to the plan this table was drawn up from: at batch 33 the hidden layer's backward is neither the pipelined body
(batch <= 32) nor the tiled GEMM (batch >= 128), so rb_debug_launch_plan reports implicit_sigma = 0 at BOTH c-b33 rows under
LEARNER_IMPLICIT_SIGMA, not 1 at 2176 (and on one device fuse_norm cannot turn 0 where implicit_sigma is possible at all: batch
<= 32 needs 10 179 slots at hidden 4096, batch >= 128 needs 15 555).  The two rows still run once more with the flag: it must be
harmless there, and test_launch_plan.py pins the 0.

Conditioning (asserted by the bodies as "ill-conditioned seed"; no row is skipped or retried).  The seed of a row is the first
one from 0 for which the ORACLE ALONE gives both learn steps a hidden_relu_margin of at least 2.5 x RELU_MARGIN and every act
call a top-two gap of at least GAP_SHARE of the support's width (`python tools/ladder_seeds.py --shape-range`, CPU only; the
margins above are what it printed).  d-b1024-h4096 has 8.4 M hidden pre-activations per step; none of the seeds 0 .. 13 clears
the margin (the widest smaller margin among them is 1.4e-08, seed 8), so that row — and no other — is `masked` in
test_learner_batches_gpu.py's sense, on the first seed that gives the act calls their gap: the oracle takes the device's hidden
ReLU decisions, and the body asserts that every decision that differs from the oracle's own sits on an oracle pre-activation
inside RELU_MARGIN and that there are no more of them than the oracle's own count of pre-activations inside RELU_MARGIN.
The conv layers' ReLU decisions are handed from the device to the oracle in every row and each differing decision is bounded by
the rounding bound of its own element (learn_steps.conv_flips).

Tolerances: helpers.assert_learn_trace_matches and head_shapes_scenarios' ACT_RTOL / ACT_ATOL, unchanged, with ONE exception
that is the oracle's own error, not the device's.  The long reductions (K = 4096 in d-h4096's output layer, K = 1024 in
c-hist16's first conv layer) needed no allowance.  The exception is the tensor class `grad_norm` in the six rows whose hidden
layer has 2 M weights and more (WIDE_NORM_ROWS): the oracle's total is torch's float32 clip_grad_norm_ reduction over those
tensors, and against the float64 norm of the oracle's OWN gradients (OracleRun.step's `exact`) it is off by, step 0 / step 1, on
the CPU:
    d-h4096 2.416e-05 / 5.795e-05    d-h4128 1.376e-05 / 4.311e-05    d-h8192       9.869e-05 / 8.450e-05
    c-b33-h2176 9.358e-05 / 8.962e-05    c-b33-h2208 5.861e-05 / 6.436e-05    d-b1024-h4096 1.462e-05 / 1.500e-05
    (for comparison d-h352 7.4e-07 / 8.2e-07, c-hist16 5.0e-07 / 4.5e-07)
which is past the helper's rtol 5e-5 (itself set to that reduction's noise at the baseline shapes) before any device runs.  For
those rows grad_norm is held against the oracle's float32 total at 4 x the largest figure above, 4 x 9.869e-05 = 3.948e-04
(NORM_RTOL_WIDE; the factor the head table uses), and — the check that carries the weight — against the float64 norm at rtol 2e-6,
which every row passes on the host interpreter and on the MI355X (all of the table's norms are under the clip of 10, asserted).

Measured on the MI355X (test_shape_range_gpu.py -s), all 19 rows and the two flagged reruns:
  - conv ReLU decisions that differ from the oracle's own: none, in any layer, step or row (0 0.0e+00 0.0e+00 throughout);
  - hidden ReLU margins of the oracle: as in the table (they are the oracle's, to the digits shown);
  - d-b1024-h4096 (masked): step 0 no hidden decision differs; step 1 one does, on |pre| = 1.118e-08, with 4 oracle pre-activations
    inside 3e-08;
  - the only misses of the first run were the six WIDE_NORM_ROWS on grad_norm against the float32 total, by 5.8e-05 .. 9.9e-05 —
    the figures above to three digits, i.e. the device norm sits on the float64 norm.
The host interpreter gives the same picture at the batch-4 rows.  It needs 2 to 10 minutes per test at hidden 4096 and above
(measured: d-h4096 119 s + 121 s, d-h4128 123 s + 243 s, d-h8192 247 s + 572 s, learn + act), so test_shape_range_emu.py runs the
batch-4 rows up to hidden 352 and those three are the device's alone."""
from collections import namedtuple

import numpy as np

import scenarios
from head_shapes_scenarios import ACT_ATOL, ACT_RTOL, GAP_SHARE, N_STATES, act_inputs, make_learner
from helpers import assert_learn_trace_matches
from learn_steps import RELU_MARGIN, OracleRun, conv_shapes, two_step_inputs
from oracle import learner_oracle as O
from rainbow_amd import _lib as L

DEFAULTS = dict(atoms=51, actions=6, multi_step=3, discount=0.99, v_min=-10.0, v_max=10.0, batch=4, history=4)
NETS = {"c": dict(architecture="canonical", hidden=64), "d": dict(architecture="data-efficient", hidden=32)}
SPARE = 2.5       # the seed search's factor on RELU_MARGIN

# id: (overrides of the defaults, what the row crosses, seed, the oracle's ReLU margin of step 0 / 1, masked)
Row = namedtuple("Row", "over crosses seed margins masked")
CASES = {
    "c-hist1": Row(dict(history=1), "split-K first layer at K 64", 1, (5.8e-05, 1.2e-05), False),
    "c-hist2": Row(dict(history=2), "split-K first layer at K 128", 0, (1.1e-05, 2.0e-06), False),
    "d-hist1": Row(dict(history=1), "first layer at K 25", 0, (5.4e-04, 7.8e-06), False),
    "d-hist3": Row(dict(history=3), "first layer at K 75", 2, (5.4e-05, 2.4e-04), False),
    "c-hist8": Row(dict(history=8), "generic convs, act rg 4", 1, (5.2e-06, 4.6e-06), False),
    "c-hist16": Row(dict(history=16), "K = RB_ACT_KMAX, act rg 1", 0, (6.9e-05, 2.8e-05), False),
    "d-hist16": Row(dict(history=16), "K 400, act rg 2", 0, (1.5e-04, 3.5e-05), False),
    "d-h1": Row(dict(hidden=1), "generic FC, act fallback", 0, (3.9e-02, 1.6e-02), False),
    "d-h3": Row(dict(hidden=3), "generic FC, act fallback", 0, (8.1e-03, 2.8e-04), False),
    "d-h128": Row(dict(hidden=128), "hsplits 1, the last", 1, (1.8e-04, 1.2e-04), False),
    "d-h160": Row(dict(hidden=160), "hsplits 2", 1, (1.3e-04, 5.0e-05), False),
    "d-h288": Row(dict(hidden=288), "hsplits 3, even", 4, (2.4e-05, 4.8e-06), False),
    "d-h352": Row(dict(hidden=352), "hsplits 3, short last split", 1, (1.1e-04, 3.5e-05), False),
    "d-h4096": Row(dict(hidden=4096), "fast_fc limit, K = RB_NL_FWD_KMAX", 2, (2.6e-06, 3.1e-07), False),
    "d-h4128": Row(dict(hidden=4128), "first generic FC above the fast_fc limit", 3, (1.3e-06, 4.7e-06), False),
    "d-h8192": Row(dict(hidden=8192), "accepted maximum", 0, (7.6e-07, 5.2e-06), False),
    "c-b33-h2176": Row(dict(batch=33, hidden=2176), "fuse_norm 1, the last", 0, (7.7e-08, 3.4e-07), False),
    "c-b33-h2208": Row(dict(batch=33, hidden=2208), "fuse_norm 0, norm from k_sumsq", 5, (1.1e-07, 5.0e-07), False),
    "d-b1024-h4096": Row(dict(batch=1024, hidden=4096), "k_fc_gemm_fwd tiles > 1024, S = 1", 2, (1.2e-08, 1.9e-08), True),
}
MAY_BE_MASKED = ("d-b1024-h4096",)
WIDE_NORM_ROWS = ("d-h4096", "d-h4128", "d-h8192", "c-b33-h2176", "c-b33-h2208", "d-b1024-h4096")     # module docstring, Tolerances
NORM_RTOL_WIDE = 4 * 9.869e-05
# (row, flag set) of the learn body: every row at the adapter's defaults, the two batch-33 rows again with the flag Agent sets
LEARN_RUNS = [(c, "default") for c in CASES] + [("c-b33-h2176", "implicit-sigma"), ("c-b33-h2208", "implicit-sigma")]
# the host interpreter's rows: batch 4, and a hidden size it gets through in seconds (module docstring, last paragraph)
EMU_CASES = [c for c, r in CASES.items() if r.over.get("batch", DEFAULTS["batch"]) == 4 and r.over.get("hidden", 0) <= 352]


def case_config(case):
    return dict(DEFAULTS, **dict(NETS[case[0]], **CASES[case].over))


def label(case, where):
    return "%s/%s [%s]" % (where, case, CASES[case].crosses)


# =============================================================================== learn
def check_learn(lib, mem, case, flagset="default", where="hip"):
    """Two consecutive learn steps of the row against the oracle: per-sample loss, gradient norm, every clipped gradient, the
    post-Adam parameters (helpers.assert_learn_trace_matches), a* and the projected m of step 0 — the method of
    test_learn_step_across_the_batch_ladder_matches_oracle, on this table."""
    row, cfgd = CASES[case], case_config(case)
    hy = scenarios.LEARN_HYPER
    inp = two_step_inputs(cfgd, row.seed)
    B, Z, H = cfgd["batch"], cfgd["atoms"], cfgd["hidden"]
    what = label(case, where) + ("" if flagset == "default" else " " + flagset)
    ad = make_learner(lib, mem, case, cfgd)
    try:
        if flagset == "implicit-sigma":
            ad.learner_flags = L.LEARNER_IMPLICIT_SIGMA
        ad.load(inp["online"], inp["target"])
        stepper = OracleRun(inp)
        got_t, want_t, exact_under_clip = {}, {}, []
        for k, st in enumerate(inp["steps"]):
            ad.reset_noise_online(st["raw_on"])
            got = ad.learn_step(st["batch"], st["raw_tg"])
            conv_masks = [ad.debug(6 + i, shp, np.float32) > 0 for i, shp in enumerate(conv_shapes(inp["cfg"], B))]
            if row.masked:
                assert case in MAY_BE_MASKED, case
                near = stepper.near_zero(k)
                o = stepper.step(k, hidden_mask=ad.debug(5, (B, 2 * H), np.float32) > 0, conv_masks=conv_masks)
                flips, flip_abs = o["want"]["hidden_mask_flips"], o["want"]["hidden_mask_flip_abs"]
                print("%s step %d: %d hidden ReLU decisions differ from the oracle's own, the largest on |pre| = %.3e; %d oracle "
                      "pre-activations inside %.0e" % (what, k, flips, flip_abs, near, RELU_MARGIN))
                assert flip_abs < RELU_MARGIN and flips <= near, (what, k, flips, flip_abs, near)
            else:
                o = stepper.step(k, conv_masks=conv_masks)
                print("%s step %d: hidden ReLU margin %.3e" % (what, k, o["want"]["hidden_relu_margin"]))
                assert o["want"]["hidden_relu_margin"] >= RELU_MARGIN, \
                    "%s: ill-conditioned seed at step %d: a hidden pre-activation within rounding noise of 0 (%.3e; " \
                    "tools/ladder_seeds.py --shape-range)" % (what, k, o["want"]["hidden_relu_margin"])
            want = o["want"]
            print("%s step %d: conv ReLU decisions that differ from the oracle's own, per layer (count, largest |pre|, largest "
                  "|pre| / bound): %s" % (what, k, ["%d %.1e %.1e" % f for f in want["conv_flips"]]))
            assert all(ratio < 1.0 for _n, _a, ratio in want["conv_flips"]), \
                "%s step %d: a conv ReLU decision differs outside its rounding bound: %s" % (what, k, want["conv_flips"])
            got_t["s%d_loss" % k], want_t["s%d_loss" % k] = got["loss"], want["loss"]
            got_t["s%d_grad_norm" % k], want_t["s%d_grad_norm" % k] = np.float32(got["grad_norm"]), np.float32(o["total"])
            exact_under_clip.append(o["exact"] <= hy["norm_clip"])
            if exact_under_clip[-1]:            # device norm against the EXACT norm of the oracle's gradients (f64), tightly
                np.testing.assert_allclose(got["grad_norm"], o["exact"], rtol=2e-6,
                                           err_msg="%s step %d: gradient norm against the f64 norm of the oracle's gradients" % (what, k))
            for name in o["clipped"]:
                got_t["s%d_grad/%s" % (k, name)], want_t["s%d_grad/%s" % (k, name)] = got["grads"][name], o["clipped"][name]
            for name, p in ad.params().items():
                got_t["s%d_param/%s" % (k, name)], want_t["s%d_param/%s" % (k, name)] = p, o["params"][name]
            if k == 0:
                a_star = ad.debug(2, (B,), np.int32)
                assert np.array_equal(a_star, want["a_star"].astype(np.int32)), \
                    "%s: a* of step 0: %s, the oracle's %s" % (what, a_star.tolist(), want["a_star"].tolist())
                np.testing.assert_allclose(ad.debug(1, (B, Z), np.float32), want["m"], rtol=1e-4, atol=1e-6,
                                           err_msg="%s: projected m of step 0" % what)
        if case in WIDE_NORM_ROWS:      # the oracle's float32 total is the noisy side here: its own measured error x 4
            for k in range(2):
                key = "s%d_grad_norm" % k
                got_n, want_n = got_t.pop(key), want_t.pop(key)
                assert exact_under_clip[k], "%s step %d: the norm is over the clip, so the float64 check did not run" % (what, k)
                np.testing.assert_allclose(got_n, want_n, rtol=NORM_RTOL_WIDE, atol=1e-7, err_msg="%s %s (float32 total of the oracle)" % (what, key))
        assert_learn_trace_matches(got_t, want_t, label=what)
    finally:
        ad.close()


# =============================================================================== act
_ACT_ORACLE = {}


def act_oracle(case, seed=None):
    """O.act per state under the shared noise, in eval mode and under the state's own noise row, with the top-two gap of the
    per-action values (float64 sum of the oracle's probabilities).  Once per row and process."""
    import torch

    import head_oracle as HO
    seed = CASES[case].seed if seed is None else seed
    if (case, seed) not in _ACT_ORACLE:
        cfg, params, raw_shared, raw_rows, states = act_inputs(case_config(case), seed)
        p = {k: torch.as_tensor(np.ascontiguousarray(v)) for k, v in params.items()}
        sup = HO.support32(cfg).astype(np.float64)
        out = {}
        for mode in ("noisy", "eval", "rows"):
            a, q, gap = np.zeros(N_STATES, np.int64), np.zeros(N_STATES, np.float32), np.zeros(N_STATES)
            for i in range(N_STATES):
                noise = None if mode == "eval" else O.make_noise(cfg, raw_shared if mode == "noisy" else raw_rows[i])
                a[i], q[i] = O.act(cfg, params, noise, states[i])
                with torch.no_grad():
                    ps = O.forward(cfg, p, noise, torch.as_tensor(states[i:i + 1]))[0].numpy().astype(np.float64)
                gap[i] = HO.top2_gap((ps * sup).sum(axis=1).reshape(1, -1))[0]
            out[mode] = dict(a=a, q=q, gap=gap)
        _ACT_ORACLE[case, seed] = out
    return _ACT_ORACLE[case, seed]


def act_gap(case, seed=None):
    ora = act_oracle(case, seed)
    return min(float(ora[k]["gap"].min()) for k in ora)


def _same(got_a, got_q, want, what):
    got_a = np.asarray(got_a, dtype=np.int64).reshape(-1)
    assert (got_a >= 0).all(), "%s: action %s — an in-launch wait of the act path expired" % (what, got_a.tolist())
    assert np.array_equal(got_a, want["a"]), "%s: actions %s, the oracle's %s" % (what, got_a.tolist(), want["a"].tolist())
    np.testing.assert_allclose(np.asarray(got_q, dtype=np.float32).reshape(-1), want["q"], rtol=ACT_RTOL, atol=ACT_ATOL,
                               err_msg="%s: q" % what)


def _same_bits(one, phases, what):
    """The two launch forms of rb_learner_act run the same bodies in the same order: equal actions, q equal as 32-bit words."""
    assert list(one[0]) == list(phases[0]), "%s: one launch chose %s, one launch per phase %s" % (what, list(one[0]), list(phases[0]))
    assert np.array_equal(one[1].view(np.uint32), phases[1].view(np.uint32)), \
        "%s: q of one launch %s, of one launch per phase %s" % (what, [x.hex() for x in one[1].astype(float)], [x.hex() for x in phases[1].astype(float)])


def check_act(lib, mem, case, monkeypatch, where="hip"):
    """Three states, noisy and eval mode: rb_learner_act (as one launch, and with RB_OPTS act_fused=0 as one launch per phase of
    the same kernel — each against the oracle, and the two against each other bit for bit), rb_learner_act_batch at n = 3,
    rb_learner_act_batch_rows at n = 3 under three noise rows — each (action, q) against O.act, one row at a time.  On the host
    interpreter both learners run one launch per phase, so the bit comparison there holds by construction."""
    cfgd, seed = case_config(case), CASES[case].seed
    cfg, params, raw_shared, raw_rows, states = act_inputs(cfgd, seed)
    ora = act_oracle(case)
    what = label(case, where)
    width = cfgd["v_max"] - cfgd["v_min"]
    gap = act_gap(case)
    print("%s act seed %d: min action gap %.3e" % (what, seed, gap))
    assert gap >= GAP_SHARE * width, "%s: ill-conditioned seed: action top-two gap %.3e" % (what, gap)
    # the three rows share no state, no noise and no value: a row mix-up in a batched call cannot pass
    for mode in ora:
        q = ora[mode]["q"].astype(np.float64)
        for i in range(N_STATES):
            for j in range(i + 1, N_STATES):
                assert abs(q[i] - q[j]) > 10 * (ACT_ATOL + ACT_RTOL * max(abs(q[i]), abs(q[j]))), \
                    "%s: ill-conditioned seed: rows %d and %d of mode %s are indistinguishable (q %r, %r)" % (what, i, j, mode, q[i], q[j])
    ad = make_learner(lib, mem, case, cfgd)
    monkeypatch.setenv("RB_OPTS", "act_fused=0")
    unfused = make_learner(lib, mem, case, cfgd)
    monkeypatch.delenv("RB_OPTS")
    m = mem
    try:
        for x in (ad, unfused):
            x.load(params, params)
            x.reset_noise_online(raw_shared)
        st = m.upload(states)
        for noisy in (1, 0):
            want = ora["noisy" if noisy else "eval"]
            got = {}
            for x, name in ((ad, "rb_learner_act"), (unfused, "rb_learner_act act_fused=0")):
                single = [x.act(s, bool(noisy)) for s in states]
                got[name] = ([s[0] for s in single], np.asarray([s[1] for s in single], dtype=np.float32))
                _same(got[name][0], got[name][1], want, "%s %s noisy=%d" % (what, name, noisy))
            _same_bits(got["rb_learner_act"], got["rb_learner_act act_fused=0"], "%s noisy=%d" % (what, noisy))
            a, q = ad.act_batch(states, bool(noisy))
            _same(a, q, want, "%s rb_learner_act_batch noisy=%d" % (what, noisy))
        # one noise sample per row, filled from the injected normals as noise_rows_scenarios.RowsContext does
        raw = m.upload(raw_rows)
        rows = m.empty((N_STATES, ad.n_noise), np.float32)
        L.check(lib, lib.rb_learner_noise_rows(ad.h, N_STATES, 0, 0, 0, m.ptr(raw), m.ptr(rows), m.stream))
        a, q = m.upload(np.full(N_STATES, -3, np.int32)), m.empty((N_STATES,), np.float32)
        L.check(lib, lib.rb_learner_act_batch_rows(ad.h, m.ptr(st), N_STATES, m.ptr(rows), m.ptr(a), m.ptr(q), m.stream))
        m.sync()
        _same(m.download(a), m.download(q), ora["rows"], "%s rb_learner_act_batch_rows" % what)
    finally:
        ad.close()
        unfused.close()


# =============================================================================== seed search (CPU, oracle only)
def oracle_margins(case, seed):
    """The oracle's hidden_relu_margin of both learn steps of `seed` (step 1 on its own post-Adam parameters of step 0)."""
    run = OracleRun(two_step_inputs(case_config(case), seed))
    return tuple(float(run.step(k)["want"]["hidden_relu_margin"]) for k in range(2))


def find_seed(case, n=14):
    """-> (found, masked, seen).  found = (seed, margins, act gap) of the first seed in [0, n) that meets the module docstring's
    conditions; where there is none, masked = the same for the first seed that gives the act calls their gap (the row then takes
    the device's hidden ReLU decisions).  seen: every seed tried."""
    cfgd, seen = case_config(case), []
    width = cfgd["v_max"] - cfgd["v_min"]
    for seed in range(n):
        margins, gap = oracle_margins(case, seed), act_gap(case, seed)
        seen.append((seed, margins, gap))
        if min(margins) >= SPARE * RELU_MARGIN and gap >= GAP_SHARE * width:
            return seen[-1], None, seen
    return None, next((s for s in seen if s[2] >= GAP_SHARE * width), None), seen
