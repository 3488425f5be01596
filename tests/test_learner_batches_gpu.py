"""GPU parity of the learn step at the batch sizes where its launch plan changes (csrc/learner_plan.h: kernels, tile shapes and
image-group sizes change at batch 33, 64, 86, 128 and 257; tests/test_launch_plan.py pins WHICH kernel each side of those
thresholds reaches, this file what those kernels compute).  The method of test_learner_gpu.py's
test_learn_step_at_baseline_shapes_matches_oracle: TWO consecutive learn steps through the C ABI against the CPU oracle on
scenarios.make_batch inputs with injected noise — per-sample loss, the gradient norm, all clipped gradients, the post-Adam
parameters (helpers.assert_learn_trace_matches, its stated tolerances), a* and the projected m of step 0.  The second step is the
one that finds a split-K arrival counter or a partial slice that did not come back to zero.

ReLU decisions.  relu' is a step: where a pre-activation lies inside the rounding noise of its f32 dot product, two correct
implementations may decide it differently, and one decision moves that sample's contribution to every upstream gradient (seen
without the treatment below, first run on the device: batch 257, one conv1 bias-gradient element of 32 off by 1.2e-7 = 0.5 %;
batch 129 at hidden 96, 16 of 32 by up to 1.7e-7, the signature of ONE conv2 decision spread over conv2's 32 input channels; the
oracle against its own f64 twin is within 1.6e-9 on those tensors, and flips one of its own conv1 decisions at batch 257).
 - Hidden layers (B x 2H pre-activations): the seed of each case is one for which the oracle alone reports a margin of at least
   RELU_MARGIN in both steps; a case without such a seed is `masked` (see the table).
 - Conv layers (B x 21 120 pre-activations in the canonical net, 2.7 M at batch 129: no seed keeps them all clear of the noise):
   EVERY case hands the device's conv ReLU decisions (rb_learner_debug_read 6 .. 8) to the oracle (learn(conv_masks=)) and
   asserts that each decision that differs from the oracle's own sits on an oracle pre-activation smaller than the worst-case
   rounding error of the two dot products that decided it, 2 (K + 1) 2^-24 (sum_k |w_k x_k| + |b|) for that very output element
   (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5: any order of a K-term f32 sum plus the bias; once for the
   device, once for the oracle).  The figures are printed: -s shows them.  Seen on the MI355X: in the canonical cases from
   batch 86 on, one or two decisions of a step differ (none at history 3 / 5, batch 63 and 33, or in the data-efficient net), on
   |pre| between 7.5e-9 and 1.4e-7 — at most 1.2e-3 of the bound, which is a worst case over every summation order and far
   above the noise; with the decisions equal every case is inside the stated tolerances."""
import numpy as np
import pytest

import scenarios
from helpers import assert_learn_trace_matches
from learn_steps import RELU_MARGIN, OracleRun, conv_flips, conv_shapes, two_step_inputs  # noqa: F401  (tools/ladder_seeds.py reads them here)


def _cfg(batch, hidden=512, history=4, architecture="canonical"):
    return dict(architecture=architecture, hidden=hidden, actions=6, atoms=51, batch=batch, multi_step=3, discount=0.99,
                history=history, v_min=-10.0, v_max=10.0)


DE = dict(architecture="data-efficient", hidden=256)
# case: (config, data seed, masked).  The seed is one for which the ORACLE ALONE reports a hidden_relu_margin of at least
# RELU_MARGIN in both steps (tools/ladder_seeds.py, CPU only; where seed 0 fails or only just passes, the seed with the
# widest margin among the first 14): below it the device and the oracle may legitimately decide a hidden
# unit's ReLU differently.  masked (no such seed in a short search): the oracle takes the device's decisions (learn(hidden_mask=))
# and the test asserts that every decision that differs from the oracle's own sits on an oracle pre-activation inside the margin.
LADDER = {
    # last batch before the data-gradient image loop; weight-gradient groups of 2 with a one-image last group; 126 forward rows in
    # 32-row chunks
    "b63": (_cfg(63), 0, False),
    # 258 images: k_conv_fwd_full<GeomC1> at 2 images per workgroup, k_conv_fwd_multi_t16 at 3 (172 online images: one group holds
    # images of both nets), k_fc_gemm_fwd with 24 tiles x split-K 8 and last row tiles of 44 and 86 live rows, k_nl_bwd<false> at
    # more than 64 rows, k_conv_dw_all with per-layer counts 2 / 3 / 3 (not uniform, last group partly empty); data gradients as ONE
    # image group of 86
    "b86": (_cfg(86), 0, False),
    # largest streamed backward under a tiled forward
    "b127": (_cfg(127), 0, False),
    # one-row GEMM tiles in forward (258 = 2 x 128 + 2, 129 = 128 + 1) and backward; weight-gradient counts 4 / 3 / 4
    "b129": (_cfg(129), 2, False),
    # image-fastest order with 5-image groups (40 groups); tiles 128 + 72; weight-gradient counts 5 / 6 / 6
    "b200": (_cfg(200), 1, False),
    # no in-launch priority write-back; 2 x 128 + 1 rows
    "b257": (_cfg(257), 2, False),
    # the accepted maximum: 1120 head workgroups, 192 GEMM tiles at split-K 1, weight-gradient counts 27 / 27 / 32
    "b1024": (_cfg(1024), 10, False),
    # 2H = 192: a 128-column tile plus a 64-column one; hsplits = 1
    "b129-h96": (_cfg(129, hidden=96), 0, False),
    # generic FC (H % 32 != 0) behind the multi-image convs, no blocked conv output
    "b129-h48": (_cfg(129, hidden=48), 0, False),
    # xs capped at 4; 512-row splits of the hidden layer's input gradient
    "b33-h1024": (_cfg(33, hidden=1024), 0, False),
    # k_conv_fwd_lds<GeomC1> as first layer with 258 images
    "b86-hist3": (_cfg(86, history=3), 0, False),
    # generic convs, k_block_copy, k_dfeat_finish, streamed FC at more than 32 rows
    "b40-hist5": (_cfg(40, history=5), 0, False),
    # k_conv_fwd_full<GeomD1>, D2 image loop
    "de-b86": (_cfg(86, **DE), 0, False),
    # the same, with the tiled backward
    "de-b129": (_cfg(129, **DE), 3, False),
    # image-fastest D2 data gradient at ipb 40; weight-gradient ipb 10
    "de-b320": (_cfg(320, **DE), 0, False),
}
# (case, flag set): every case at the adapter's defaults; batch 129 and 257 again with the flag Agent sets on one device — the
# plan reports implicit_sigma=1 on the tiled backward at both.  rb_learner_clip_adam run as a launch of its own materialises the
# sigma gradient the backward left out (k_materialize_sigma) before it clips, so the adapter reads it back from grads_dev like
# every other gradient and no further flag is needed.
# Short last image groups in the data-gradient kernels: at default options there are none (a batch that no count divides into a
# multiple of 8 groups gets ONE group, tests/test_launch_plan.py), so two more runs reach them through RB_OPTS dx_ipb —
# k_conv_dx_t16_multi<GeomC3 / GeomC2> with 65 groups of 2 at batch 129 (a one-image last group) and 52 groups of 5 at batch 257 (a
# two-image last group), and k_conv_dx_lds<GeomD2, MULTI> with 13 groups of 7 at batch 86 (a two-image last group).
RUNS = [(c, "default") for c in LADDER] + [("b129", "implicit-sigma"), ("b257", "implicit-sigma"),
                                           ("b129", "dx_ipb=2"), ("b257", "dx_ipb=5"), ("de-b86", "dx_ipb=7")]


def case_inputs(case, seed=None):
    """The seeded inputs of a case: both nets' parameters and, per step, the raw noise draws and the batch (seed: the table's)."""
    return two_step_inputs(LADDER[case][0], LADDER[case][1] if seed is None else seed)


@pytest.fixture(scope="module")
def hip():
    from rainbow_amd import _lib
    return _lib.load()


@pytest.mark.gpu
@pytest.mark.parametrize("case,flagset", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_learn_step_across_the_batch_ladder_matches_oracle(hip, monkeypatch, case, flagset):
    from cabi_adapter import CAbiLearnAdapter, TorchMem
    from rainbow_amd import _lib as L
    cfgd, _seed, masked = LADDER[case]
    monkeypatch.setitem(scenarios.LEARN_CONFIGS, case, cfgd)
    hy = scenarios.LEARN_HYPER
    inp = case_inputs(case)
    B, Z, H = cfgd["batch"], cfgd["atoms"], cfgd["hidden"]
    if flagset.startswith("dx_ipb="):
        monkeypatch.setenv("RB_OPTS", flagset)
    ad = CAbiLearnAdapter(hip, TorchMem(), case)
    if flagset == "implicit-sigma":
        ad.learner_flags = L.LEARNER_IMPLICIT_SIGMA
    ad.load(inp["online"], inp["target"])
    stepper = OracleRun(inp)
    got_t, want_t = {}, {}
    for k, st in enumerate(inp["steps"]):
        ad.reset_noise_online(st["raw_on"])
        got = ad.learn_step(st["batch"], st["raw_tg"])
        conv_masks = [ad.debug(6 + i, shp, np.float32) > 0 for i, shp in enumerate(conv_shapes(inp["cfg"], B))]
        if masked:
            near = stepper.near_zero(k)
            o = stepper.step(k, hidden_mask=ad.debug(5, (B, 2 * H), np.float32) > 0, conv_masks=conv_masks)
            flips, flip_abs = o["want"]["hidden_mask_flips"], o["want"]["hidden_mask_flip_abs"]
            print("%s step %d: %d ReLU decisions differ from the oracle's own, the largest on |pre| = %.3e; %d oracle pre-activations "
                  "inside %.0e" % (case, k, flips, flip_abs, near, RELU_MARGIN))
            assert flip_abs < RELU_MARGIN and flips <= near, (k, flips, flip_abs, near)
        else:
            o = stepper.step(k, conv_masks=conv_masks)
            assert o["want"]["hidden_relu_margin"] >= RELU_MARGIN, \
                "ill-conditioned seed at step %d: a hidden pre-activation within rounding noise of 0 (tools/ladder_seeds.py)" % k
        want = o["want"]
        print("%s/%s step %d: conv ReLU decisions that differ from the oracle's own, per layer (count, largest |pre|, largest |pre| / "
              "bound): %s" % (case, flagset, k, ["%d %.1e %.1e" % f for f in want["conv_flips"]]))
        assert all(ratio < 1.0 for _n, _a, ratio in want["conv_flips"]), want["conv_flips"]
        got_t["s%d_loss" % k], want_t["s%d_loss" % k] = got["loss"], want["loss"]
        got_t["s%d_grad_norm" % k], want_t["s%d_grad_norm" % k] = np.float32(got["grad_norm"]), np.float32(o["total"])
        if o["exact"] <= hy["norm_clip"]:   # device norm against the EXACT norm of the oracle's gradients (f64), tightly
            np.testing.assert_allclose(got["grad_norm"], o["exact"], rtol=2e-6)
        for name in o["clipped"]:
            got_t["s%d_grad/%s" % (k, name)], want_t["s%d_grad/%s" % (k, name)] = got["grads"][name], o["clipped"][name]
        for name, p in ad.params().items():
            got_t["s%d_param/%s" % (k, name)], want_t["s%d_param/%s" % (k, name)] = p, o["params"][name]
        if k == 0:
            assert np.array_equal(ad.debug(2, (B,), np.int32), want["a_star"].astype(np.int32))
            np.testing.assert_allclose(ad.debug(1, (B, Z), np.float32), want["m"], rtol=1e-4, atol=1e-6)
    assert_learn_trace_matches(got_t, want_t, label="hip/%s/%s" % (case, flagset))
    ad.close()
