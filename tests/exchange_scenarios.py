"""The replica exchange (rb_learner_set_exchange, k_pack_factors, rb_learner_finish_grads = k_finish_grads_tiled, and the learn step
they reshape) over world size, batch and layer shapes: two tables and their bodies, run on the host interpreter
(test_exchange_shapes_emu.py) and on the device (test_exchange_shapes_gpu.py) through the C ABI.  tests/test_exchange_gpu.py and
test_learner_emu.py's world 3 / 8 run stay as they are; they run at batch 32, 51 atoms, 6 actions, history 4 only.

Every row: 51 atoms, 6 actions, multi_step 3, discount 0.99, support [-10, 10], batch 4, history 4, hidden 32 on the
data-efficient stack ("d-", F 576) or hidden 64 on the canonical one ("c-", F 3136) unless its id says otherwise.

A. rb_learner_finish_grads against a float64 fold of GIVEN blocks (check_finish).  finish_grads is a pure function of the gathered
buffer: one real learn call per handle arms it (and its packed block is checked bit for bit against what it was packed from),
then the test overwrites the gathered buffer with `world` synthetic rank blocks — gradient-side segments (dlogits, dh, conv
gradients) of rank r scaled by its own factor in 1e-3 .. 1e1, so a rank mix-up shows; h and feat >= 0 with ReLU's zeros; the whole
buffer pre-filled with NaN, so every alignment gap stays NaN — and every FC tensor and the conv range are held against numpy float64:
    g_mu = (1/W) sum_r dY_r^T X_r            g_sigma = (1/W) sum_r (dY_r^T X_r) o (eps_out_r x eps_in_r)
    g_bmu = (1/W) sum_r colsum dY_r          g_bsigma = (1/W) sum_r colsum dY_r o eps_out_r         conv range: the rank mean
(value rows read h[:, :H], advantage rows h[:, H:]; the noise offsets are rb_learner_noise_layout's).  One rank's block is six
segments, each rounded up to 64 floats:  dlogits [B][NZ] | h [B][2H] | dh [B][2H] | feat [B][F] | noise [n_noise] | conv grads.
Bound per element (any-order summation, Higham eq. 3.5, the form learn_steps.conv_flips uses), u = 2^-24:
    2 (B + W + c) u mag,  mag = the same fold over absolute values,  c = 2 (mu, bias_mu), 3 (bias_sigma), 4 (sigma);
    conv range: 2 (W + 1) u mag.
B products and B - 1 adds per rank, W adds of the rank fold, c for the noise product(s), the 1 / W factor (itself rounded to
float32) and its multiplication.  Derived, not tuned: observed / bound of every row on both backends is recorded in
profiles/exchange_bounds.txt; a ratio of 1 or more fails.
Also per row: every gradient float finite (no NaN gap consumed); two handles that saw the same gathered buffer but ran their own
learn call (other batch, other noise) bit-identical in gradients, norm and post-Adam parameters; the norm rb_learner_clip_adam
reports against the float64 norm of the device's own gradient at rtol 2e-6 (shape_range_scenarios' figure); the guard bands of
every caller-owned buffer (guarded_mem) intact.
A finding of the pack check: the conv segment is the leading small_floats of the flat gradient, alignment padding between the conv
tensors included (32 floats on the data-efficient stack).  The learn call writes the tensors' elements only — the padding of the
NaN-filled local block is asserted to stay NaN, and the segment is compared on the tensors' elements — while finish_grads folds
and squares the whole range; a caller must therefore allocate its local block zero-filled (rainbow_amd.dist does;
include/rainbow_hip.h says so), and the synthetic blocks hold zero there.

  row             world  crosses
  a-d-w2              2  N = 64 in a 128-row tile; F = 4.5 column tiles; one slab with 28 masked rows; output-layer K = 32 in a
                         512-column workgroup (seven of eight waves leave)
  a-d-w3-b1           3  rpb 1: every clamp lands on row 0; scale 1/3
  a-d-w5              5  bias column sums: rank 4 is the second trip of group 0
  a-d-w9              9  the conv fold's second 8-wide trip, one live rank
  a-d-w64            64  the accepted maximum: M = 256, LDS parking rows 0 .. 63, eight full trips
  a-d-w2-b33          2  spr 2, second slab with one live row; the output layer's row loop twice
  a-d-w3-b64          3  two full slabs per rank
  a-d-w2-h96          2  N = 192: 1.5 row tiles
  a-d-w2-h544         2  output-layer K = 544: a second 512-column workgroup with 32 live columns; N = 8.5 row tiles
  a-c-w2              2  F = 3136 (24.5 column tiles), N = 128 exactly
  a-d-w2-z2-a1        2  Z = 2, NZ = 4
  a-d-w2-z65-a8       2  five value tiles (last: 1 row), 33 advantage tiles (last: 8 rows), ldy = 585
  a-d-w2-hist1        2  the smallest conv range

B. Two learn steps with the exchange armed against the oracle fed the MEAN gradient (check_learn): test_exchange_gpu.py's body
on `world` handles with their own batch and noise — per-rank loss, gradients, norm and post-Adam parameters through
helpers.assert_learn_trace_matches, unchanged; all handles bit-identical — along the switches `exch` makes in
csrc/learner_plan.h plan_fc_bwd (tests/test_launch_plan.py pins them with world = 2):

  row             world  crosses                                                          seed  ReLU margin, step 0 / 1 (min over ranks)
  e-d-w2              2  tall output-layer dX, M32 hidden-layer dX, dW grids 0               0  1.2e-04 / 1.5e-04
  e-d-w3-b33          3  z_tall off; the M64 input-gradient bodies                           0  4.1e-05 / 3.9e-05
  e-d-w2-b129         2  tiled forward GEMM + streamed backward, three 64-row chunks,        0  3.4e-06 / 1.7e-06
                         the last of one row
  e-d-w2-h160         2  hsplits 2: lazy dfeat                                               0  7.8e-06 / 1.6e-05
  e-c-w2              2  canonical                                                           0  9.1e-06 / 4.9e-06
  e-c-w2-hist8        2  fast_conv 0: k_gemm convs, k_block_copy, k_dfeat_finish             0  1.0e-05 / 4.0e-05
  e-d-w2-z65-a8       2  k_head<2>, odd NZ                                                   0  2.5e-05 / 5.6e-05
e-d-w2 runs once more with the flags Agent sets on one device (deferred update, implicit sigma): harmless, the plan turns what
they ask for off under `exch`.

Conditioning (asserted as "ill-conditioned seed"; no row is skipped, masked or retried): the seed of a row is the first one from 0
for which the ORACLE ALONE gives every rank, in both steps, a hidden_relu_margin of at least 2.5 x RELU_MARGIN
(`python tools/ladder_seeds.py --exchange`, CPU only; the margins above are what it printed).  Every row has such a seed among
0 .. 13 (seed 0 throughout), so none is masked.  The conv layers' ReLU decisions are handed from each rank's device run to the
oracle and each differing decision is judged by learn_steps.conv_flips.

Where the rows run: the device runs every row.  The host interpreter runs every A row (finish_grads takes seconds there, about
ten at world 64) and the B rows it finishes in about a minute; e-d-w2-b129 (over 100 s for ONE of its four learn calls),
e-d-w3-b33 (six learn calls at batch 33: 174 s, measured, the slowest test of the CPU suite by 50 s; it passed every tensor) and
e-c-w2-hist8 (every conv on the interpreted k_gemm) are the device's alone (EMU_LEARN_CASES)."""
import ctypes as C
from collections import namedtuple

import numpy as np

import scenarios
from head_shapes_scenarios import make_learner
from helpers import assert_learn_trace_matches
from learn_steps import RELU_MARGIN, conv_flips, conv_shapes
from oracle import learner_oracle as O
from rainbow_amd import _lib as L

DEFAULTS = dict(atoms=51, actions=6, multi_step=3, discount=0.99, v_min=-10.0, v_max=10.0, batch=4, history=4)
NETS = {"c": dict(architecture="canonical", hidden=64), "d": dict(architecture="data-efficient", hidden=32)}
SPARE = 2.5       # the seed search's factor on RELU_MARGIN
RB_ERR_STATE = -4  # include/rainbow_hip.h
U = 2.0 ** -24

# ------------------------------------------------------------------------------------------------------------- table A
FinishRow = namedtuple("FinishRow", "world over crosses")
FINISH_CASES = {
    "a-d-w2": FinishRow(2, {}, "N 64 in a 128-row tile, 28 masked rows, K 32 in a 512-column workgroup"),
    "a-d-w3-b1": FinishRow(3, dict(batch=1), "rpb 1, scale 1/3"),
    "a-d-w5": FinishRow(5, {}, "bias column sums: second trip of group 0"),
    "a-d-w9": FinishRow(9, {}, "conv fold: second trip, one live rank"),
    "a-d-w64": FinishRow(64, {}, "accepted maximum"),
    "a-d-w2-b33": FinishRow(2, dict(batch=33), "spr 2, one live row in the second slab"),
    "a-d-w3-b64": FinishRow(3, dict(batch=64), "two full slabs per rank"),
    "a-d-w2-h96": FinishRow(2, dict(hidden=96), "N 192: 1.5 row tiles"),
    "a-d-w2-h544": FinishRow(2, dict(hidden=544), "output-layer K 544: second workgroup, 32 live columns"),
    "a-c-w2": FinishRow(2, {}, "F 3136, N 128 exactly"),
    "a-d-w2-z2-a1": FinishRow(2, dict(atoms=2, actions=1), "Z 2, NZ 4"),
    "a-d-w2-z65-a8": FinishRow(2, dict(atoms=65, actions=8), "short last row tiles, ldy 585"),
    "a-d-w2-hist1": FinishRow(2, dict(history=1), "the smallest conv range"),
}
BOUND_C = {"weight_mu": 2, "bias_mu": 2, "bias_sigma": 3, "weight_sigma": 4}

# ------------------------------------------------------------------------------------------------------------- table B
LearnRow = namedtuple("LearnRow", "world over crosses seed margins")
LEARN_CASES = {
    "e-d-w2": LearnRow(2, {}, "tall output-layer dX, M32 hidden-layer dX, dW grids 0", 0, (1.2e-04, 1.5e-04)),
    "e-d-w3-b33": LearnRow(3, dict(batch=33), "z_tall off, M64 input-gradient bodies", 0, (4.1e-05, 3.9e-05)),
    "e-d-w2-b129": LearnRow(2, dict(batch=129), "tiled forward GEMM + streamed backward", 0, (3.4e-06, 1.7e-06)),
    "e-d-w2-h160": LearnRow(2, dict(hidden=160), "hsplits 2: lazy dfeat", 0, (7.8e-06, 1.6e-05)),
    "e-c-w2": LearnRow(2, {}, "canonical", 0, (9.1e-06, 4.9e-06)),
    "e-c-w2-hist8": LearnRow(2, dict(history=8), "fast_conv 0", 0, (1.0e-05, 4.0e-05)),
    "e-d-w2-z65-a8": LearnRow(2, dict(atoms=65, actions=8), "k_head<2>, odd NZ", 0, (2.5e-05, 5.6e-05)),
}
AGENT_FLAGS = L.LEARNER_DEFER_UPDATE | L.LEARNER_IMPLICIT_SIGMA      # what Agent sets on one device (agent.py)
LEARN_RUNS = [(c, "default") for c in LEARN_CASES] + [("e-d-w2", "agent-flags")]
# the host interpreter's rows (module docstring, last paragraph)
EMU_LEARN_CASES = [c for c in LEARN_CASES if c not in ("e-d-w2-b129", "e-d-w3-b33", "e-c-w2-hist8")]
EMU_LEARN_RUNS = [r for r in LEARN_RUNS if r[0] in EMU_LEARN_CASES]


def case_config(case):
    row = FINISH_CASES[case] if case in FINISH_CASES else LEARN_CASES[case]
    return dict(DEFAULTS, **dict(NETS[case[2]], **row.over))


def make_batch(cfgd, seed):
    """scenarios.make_batch indexes row 2: a batch below 3 is the head of a batch-4 one."""
    if cfgd["batch"] >= 3:
        return scenarios.make_batch(cfgd, seed)
    return {k: v[:cfgd["batch"]].copy() for k, v in scenarios.make_batch(dict(cfgd, batch=4), seed).items()}


def align64(n):
    return (n + 63) // 64 * 64


def block_layout(B, NZ, H, F, n_noise, small_floats):
    """The exchange block restated: ({segment: (offset, floats)}, total)."""
    out, off = {}, 0
    for name, n in (("dlogits", B * NZ), ("h", B * 2 * H), ("dh", B * 2 * H), ("feat", B * F), ("noise", n_noise), ("conv", small_floats)):
        out[name] = (off, n)
        off = align64(off + n)
    return out, off


def fill(buf, arr):
    """Overwrite a caller-owned buffer (numpy array or torch tensor) with a host array of the same size."""
    if isinstance(buf, np.ndarray):
        buf[...] = arr.reshape(buf.shape)
    else:
        import torch
        buf.copy_(torch.from_numpy(np.ascontiguousarray(arr)).reshape(buf.shape))


def exchange_layout(lib, ad):
    f, off, n = C.c_int64(0), C.c_int64(-1), C.c_int64(0)
    L.check(lib, lib.rb_learner_exchange_layout(ad.h, C.byref(f), C.byref(off), C.byref(n)))
    return f.value, off.value, n.value


# =============================================================================== A: finish_grads on given blocks
def synthetic_blocks(lay, stride, world, dims, conv_live, seed):
    """`world` rank blocks in one NaN-filled [world][stride] buffer, and the segments as arrays per rank.  conv_live: which floats of
    the conv range belong to a tensor; the alignment padding between the conv tensors travels with the range and is folded with
    it, so it holds what a caller's zero-initialised block holds there: zero."""
    B, NZ, H, F = dims
    rs = np.random.RandomState(seed)
    buf = np.full((world, stride), np.nan, dtype=np.float32)
    factors = 10.0 ** rs.uniform(-3.0, 1.0, size=world)
    ranks = []
    for r in range(world):
        s = np.float32(factors[r])
        seg = dict(dlogits=(rs.randn(B, NZ) * s).astype(np.float32), h=np.maximum(rs.randn(B, 2 * H), 0.0).astype(np.float32),
                   dh=(rs.randn(B, 2 * H) * s).astype(np.float32), feat=np.maximum(rs.randn(B, F), 0.0).astype(np.float32),
                   noise=rs.randn(lay["noise"][1]).astype(np.float32), conv=(rs.randn(lay["conv"][1]) * s * conv_live).astype(np.float32))
        for name, a in seg.items():
            off, n = lay[name]
            assert a.size == n, (name, a.size, n)
            buf[r, off:off + n] = a.ravel()
        ranks.append(seg)
    return buf, ranks


def fold_reference(ranks, noise_layout, dims, Z):
    """-> {tensor: (float64 value, float64 magnitude, c)} of every FC tensor and "conv" (c = None) from the rank segments."""
    B, NZ, H, F = dims
    W = len(ranks)
    streams = {"fc_z_v": lambda s: (s["dlogits"][:, :Z], s["h"][:, :H]), "fc_z_a": lambda s: (s["dlogits"][:, Z:], s["h"][:, H:]),
               "fc_h_v": lambda s: (s["dh"][:, :H], s["feat"]), "fc_h_a": lambda s: (s["dh"][:, H:], s["feat"])}
    out = {}
    for name, pick in streams.items():
        acc = {k: [0.0, 0.0] for k in BOUND_C}
        for s in ranks:
            dy, x = (a.astype(np.float64) for a in pick(s))
            eo_off, eo_shape = noise_layout[name + ".eps_out"]
            ei_off, ei_shape = noise_layout[name + ".eps_in"]
            eo = s["noise"][eo_off:eo_off + eo_shape[0]].astype(np.float64)
            ei = s["noise"][ei_off:ei_off + ei_shape[0]].astype(np.float64)
            assert eo.size == dy.shape[1] and ei.size == x.shape[1], (name, eo.size, dy.shape, ei.size, x.shape)
            g, ga = dy.T @ x, np.abs(dy).T @ np.abs(x)
            ee = np.outer(eo, ei)
            cs, csa = dy.sum(axis=0), np.abs(dy).sum(axis=0)
            for key, v, m in (("weight_mu", g, ga), ("weight_sigma", g * ee, ga * np.abs(ee)), ("bias_mu", cs, csa),
                              ("bias_sigma", cs * eo, csa * np.abs(eo))):
                acc[key][0] = acc[key][0] + v
                acc[key][1] = acc[key][1] + m
        for key, (v, m) in acc.items():
            out["%s.%s" % (name, key)] = (v / W, m / W, BOUND_C[key])
    conv = np.stack([s["conv"].astype(np.float64) for s in ranks])
    out["conv"] = (conv.sum(axis=0) / W, np.abs(conv).sum(axis=0) / W, None)
    return out


def worst_ratio(got, want, mag, bound_factor):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    bound = bound_factor * U * mag
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


def check_finish(lib, Mem, case, where="hip"):
    """Module docstring, A.  Mem: guarded_mem.GuardedNumpyMem / GuardedTorchMem."""
    row, cfgd = FINISH_CASES[case], case_config(case)
    cfg = O.Config(**cfgd)
    world, B, Z, H = row.world, cfgd["batch"], cfgd["atoms"], cfgd["hidden"]
    NZ = Z * (cfgd["actions"] + 1)
    shapes = conv_shapes(cfg, B)
    F = int(np.prod(shapes[-1][1:]))
    what = "%s/%s [%s]" % (where, case, row.crosses)
    m = Mem()
    ads = [make_learner(lib, m, case + "-%d" % i, cfgd) for i in range(2)]
    try:
        stride, small_off, small = exchange_layout(lib, ads[0])
        lay, total = block_layout(B, NZ, H, F, ads[0].n_noise, small)
        assert total == stride and small_off == 0, "%s: the block layout restated here has %d floats, factor_floats is %d" % (what, total, stride)
        noise_layout = {k: v for k, v in _noise_layout(lib, ads[0]).items()}
        online, target = O.init_params(cfg, 31), O.init_params(cfg, 32)
        draws = O.noise_draw_count(cfg)
        local = [m.empty((stride,), np.float32) for _ in ads]
        gathered = [m.empty((world * stride,), np.float32) for _ in ads]
        conv_live = np.zeros(small, dtype=bool)
        for name, (off, shape) in ads[0].layout.items():
            if name.startswith("convs."):
                conv_live[off:off + int(np.prod(shape))] = True
        # ---- one real learn call per handle (own batch, own noise) arms it; its packed block, bit for bit
        for i, ad in enumerate(ads):
            ad.load(online, target)
            L.check(lib, lib.rb_learner_set_exchange(ad.h, world, m.ptr(local[i]), m.ptr(gathered[i])))
            fill(local[i], np.full(stride, np.nan, dtype=np.float32))
            rs = np.random.RandomState(500 + i)
            raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
            ad.reset_noise_online(raw_on)
            ad.learn_only(make_batch(cfgd, 600 + i), raw_tg)
            m.sync()
            blk = m.download(local[i])
            packed = {name: blk[off:off + n] for name, (off, n) in lay.items()}
            srcs = dict(h=ad.debug(5, (B, 2 * H), np.float32), feat=ad.debug(6 + len(shapes) - 1, shapes[-1], np.float32),
                        noise=m.download(ad.z_on), conv=m.download(ad.grads)[:small])
            for name, src in srcs.items():
                live = conv_live if name == "conv" else np.ones(src.size, dtype=bool)
                assert np.array_equal(packed[name].view(np.uint32)[live], src.ravel().view(np.uint32)[live]), \
                    "%s handle %d: the packed %s segment is not its source bit for bit" % (what, i, name)
            assert np.isfinite(packed["dlogits"]).all() and np.isfinite(packed["dh"]).all(), "%s handle %d: packed factors" % (what, i)
            gaps = np.ones(stride, dtype=bool)
            for off, n in lay.values():
                gaps[off:off + n] = False
            gaps[lay["conv"][0]:lay["conv"][0] + small] = ~conv_live
            assert np.isnan(blk[gaps]).all(), "%s handle %d: the learn call wrote into an alignment gap of its block" % (what, i)
        # ---- the gathered buffer: `world` synthetic blocks, NaN between the segments
        buf, ranks = synthetic_blocks(lay, stride, world, (B, NZ, H, F), conv_live, 700 + world)
        for al in gathered:
            fill(al, buf)
        raw, norms, params = [], [], []
        for ad in ads:
            L.check(lib, lib.rb_learner_finish_grads(ad.h, m.stream))
            m.sync()
            raw.append(m.download(ad.grads).copy())
            out = ad.finish_step()
            norms.append(out["grad_norm"])
            params.append(m.download(ad.p_on.detach() if hasattr(ad.p_on, "detach") else ad.p_on).copy())
        # ---- two handles, one gathered buffer: nothing local leaks into the fold
        assert np.array_equal(raw[0].view(np.uint32), raw[1].view(np.uint32)), "%s: the two handles' gradients differ" % what
        assert norms[0] == norms[1], "%s: the two handles' norms differ: %r, %r" % (what, norms[0], norms[1])
        assert np.array_equal(params[0].view(np.uint32), params[1].view(np.uint32)), "%s: the two handles' post-Adam parameters differ" % what
        got = ads[0]._unflat(raw[0])
        got["conv"] = raw[0][:small]
        ref = fold_reference(ranks, noise_layout, (B, NZ, H, F), Z)
        covered = int(conv_live.sum()) + sum(int(np.prod(ads[0].layout[n][1])) for n in ref if n != "conv")
        assert covered == sum(int(np.prod(s)) for _o, s in ads[0].layout.values()), "%s: a tensor is compared twice or not at all" % what
        worst = {}
        for name, (want, mag, c) in ref.items():
            g = got[name]
            assert np.isfinite(g).all(), "%s: %s holds a non-finite value (a NaN gap was consumed)" % (what, name)
            factor = 2.0 * (world + 1) if c is None else 2.0 * (B + world + c)
            ratio = worst_ratio(g, want.reshape(g.shape), mag.reshape(g.shape), factor)
            kind = "conv" if c is None else name.split(".")[1]
            worst[kind] = max(worst.get(kind, 0.0), ratio)
            assert ratio < 1.0, "%s: %s is %.3f of its rounding bound away from the float64 fold" % (what, name, ratio)
        print("exchange_bounds %s %s %s" % (where, case, " ".join("%s %.4f" % kv for kv in sorted(worst.items()))))
        # ---- the norm of the optimiser pass against the float64 norm of the device's own gradient
        exact = np.sqrt(sum(float((got[n].astype(np.float64) ** 2).sum()) for n in ref))
        print("exchange_bounds %s %s norm %.3e" % (where, case, abs(norms[0] - exact) / exact))
        np.testing.assert_allclose(norms[0], exact, rtol=2e-6, err_msg="%s: gradient norm against the f64 norm of the device's gradient" % what)
        n_blocks, bad = m.check()
        assert not bad, "%s: guard bands written: %s" % (what, bad)
    finally:
        for ad in ads:
            lib.rb_learner_set_exchange(ad.h, 1, None, None)
            ad.close()


def _noise_layout(lib, ad):
    from cabi_adapter import query_layout
    return query_layout(lib, ad.cfg, lib.rb_learner_noise_layout)


# =============================================================================== host checks (no launch)
def check_refusals(lib, Mem, where="hip"):
    """World 0 and 65, finish_grads without a pending learn call, a handle without fast_fc: refused, each with its message."""
    m = Mem()
    cfgd = dict(DEFAULTS, **NETS["d"])
    ad = make_learner(lib, m, "refusals", cfgd)
    odd = make_learner(lib, m, "refusals-h3", dict(cfgd, hidden=3))
    try:
        stride = exchange_layout(lib, ad)[0]
        lo, al = m.empty((stride,), np.float32), m.empty((2 * stride,), np.float32)
        for world in (0, 65):
            assert lib.rb_learner_set_exchange(ad.h, world, m.ptr(lo), m.ptr(al)) != 0, "%s: world %d accepted" % (where, world)
            assert b"world must be in [1,64]" in lib.rb_last_error()
        L.check(lib, lib.rb_learner_set_exchange(ad.h, 64, m.ptr(lo), m.ptr(al)))       # (arming alone touches no buffer)
        L.check(lib, lib.rb_learner_set_exchange(ad.h, 2, m.ptr(lo), m.ptr(al)))
        assert lib.rb_learner_finish_grads(ad.h, m.stream) != 0, "%s: finish_grads without a learn call accepted" % where
        assert b"no learn call with a pending exchange" in lib.rb_last_error()
        lo3, al3 = m.empty((exchange_layout(lib, odd)[0],), np.float32), m.empty((2 * exchange_layout(lib, odd)[0],), np.float32)
        assert lib.rb_learner_set_exchange(odd.h, 2, m.ptr(lo3), m.ptr(al3)) == RB_ERR_STATE, "%s: hidden 3 accepted" % where
        msg = lib.rb_last_error()
        assert b"streamed noisy-linear kernels" in msg and b"rb_learner_grads_modified" in msg, msg
    finally:
        for x in (ad, odd):
            lib.rb_learner_set_exchange(x.h, 1, None, None)
            x.close()


def check_slot_limit(lib, Mem, where="hip"):
    """rb_learner_finish_grads writes 8 sum-of-squares slots per tile workgroup and one per conv slice; 16 384 exist.  Canonical,
    hidden 4096, batch 4: 8 * 64 * 25 + 64 * 25 = 14 400 for the hidden layer and the conv range, and 8 * 8 * (4 + ceil(51 A / 16))
    for the output layer — 1536 at 6 actions (15 936: accepted), 3968 at 18 (18 368: refused where the exchange is armed, not
    after the learn call).  Creating the handle allocates; nothing is launched."""
    m = Mem()
    for actions, slots in ((18, 18368), (6, 15936)):
        cfgd = dict(DEFAULTS, **dict(NETS["c"], hidden=4096, actions=actions))
        ad = make_learner(lib, m, "slots-a%d" % actions, cfgd)
        try:
            stride = exchange_layout(lib, ad)[0]
            lo, al = m.empty((stride,), np.float32), m.empty((2 * stride,), np.float32)
            rc = lib.rb_learner_set_exchange(ad.h, 2, m.ptr(lo), m.ptr(al))
            if slots > 16384:
                assert rc == RB_ERR_STATE, "%s: %d actions (%d slots) accepted: rc %d" % (where, actions, slots, rc)
                msg = lib.rb_last_error()
                assert str(slots).encode() in msg and b"16384" in msg and b"rb_learner_grads_modified" in msg, msg
            else:
                assert rc == 0, "%s: %d actions (%d slots) refused: %s" % (where, actions, slots, lib.rb_last_error())
        finally:
            lib.rb_learner_set_exchange(ad.h, 1, None, None)
            ad.close()


# =============================================================================== B: two learn steps, the oracle on the mean
def learn_inputs(cfgd, world, seed):
    """The seeded inputs of a row: both nets' parameters and, per step and rank, the raw noise draws and the batch."""
    cfg = O.Config(**cfgd)
    draws = O.noise_draw_count(cfg)
    rs = np.random.RandomState(2000 + seed)
    steps = [[dict(raw_on=rs.randn(draws).astype(np.float32), raw_tg=rs.randn(draws).astype(np.float32),
                   batch=make_batch(cfgd, 9000 + 100 * seed + 10 * k + r)) for r in range(world)] for k in range(2)]
    return dict(cfg=cfg, online=O.init_params(cfg, 901 + 2 * seed), target=O.init_params(cfg, 902 + 2 * seed), steps=steps)


class MeanOracle:
    """The oracle's two steps of `world` replicas: every rank's gradient on the shared parameters, their mean (float64 sum,
    rounded, over float32 world — test_exchange_gpu.py's), clip, Adam."""

    def __init__(self, inp):
        hy = scenarios.LEARN_HYPER
        self.inp, self.hy, self.online = inp, hy, inp["online"]
        self.adam = O.AdamOracle(inp["online"], hy["lr"], hy["adam_eps"])

    def step(self, k, conv_masks=None):
        cfg, world = self.inp["cfg"], len(self.inp["steps"][k])
        per_rank = []
        for r, st in enumerate(self.inp["steps"][k]):
            masks = None if conv_masks is None else conv_masks[r]
            want = O.learn(cfg, self.online, self.inp["target"], O.make_noise(cfg, st["raw_on"]), O.make_noise(cfg, st["raw_tg"]),
                           st["batch"], conv_masks=masks)
            if masks is not None:
                want["conv_flips"] = conv_flips(cfg, self.online, want.pop("conv_pre"), want.pop("conv_in"), masks)
            per_rank.append(want)
        gmean = {n: sum(pr["grads"][n].astype(np.float64) for pr in per_rank).astype(np.float32) / np.float32(world)
                 for n in per_rank[0]["grads"]}
        total, clipped = O.clip_grads(gmean, self.hy["norm_clip"])
        self.online = self.adam.step(clipped)
        return dict(per_rank=per_rank, total=total, clipped=clipped, params={n: v.copy() for n, v in self.online.items()},
                    margin=min(float(pr["hidden_relu_margin"]) for pr in per_rank))


def check_learn(lib, Mem, case, flagset="default", where="hip"):
    """Module docstring, B.  Mem: cabi_adapter.NumpyMem / TorchMem."""
    row, cfgd = LEARN_CASES[case], case_config(case)
    world, B = row.world, cfgd["batch"]
    inp = learn_inputs(cfgd, world, row.seed)
    what = "%s/%s [%s]" % (where, case, row.crosses) + ("" if flagset == "default" else " " + flagset)
    m = Mem()
    ads = [make_learner(lib, m, case + "-%d" % r, cfgd) for r in range(world)]
    try:
        stride = exchange_layout(lib, ads[0])[0]
        # include/rainbow_hip.h, rb_learner_set_exchange: "allocate the local block zero-filled" (the padding between the conv tensors
        # is folded with the conv segment) — uploaded as zeros, so that a Mem whose empty() is not zero keeps the contract
        local = [m.upload(np.zeros(stride, dtype=np.float32)) for _ in ads]
        gathered = [m.empty((world * stride,), np.float32) for _ in ads]
        for ad, lo, al in zip(ads, local, gathered):
            if flagset == "agent-flags":
                ad.learner_flags = AGENT_FLAGS
            ad.load(inp["online"], inp["target"])
            L.check(lib, lib.rb_learner_set_exchange(ad.h, world, m.ptr(lo), m.ptr(al)))
        oracle = MeanOracle(inp)
        got_t, want_t = {}, {}
        for k in range(2):
            masks = []
            for ad, st in zip(ads, inp["steps"][k]):
                ad.reset_noise_online(st["raw_on"])
                ad.learn_only(st["batch"], st["raw_tg"])
                masks.append([ad.debug(6 + i, shp, np.float32) > 0 for i, shp in enumerate(conv_shapes(inp["cfg"], B))])
            m.sync()
            cat = np.concatenate([m.download(lo) for lo in local])           # the all-gather
            for ad, al in zip(ads, gathered):
                fill(al, cat)
                L.check(lib, lib.rb_learner_finish_grads(ad.h, m.stream))
            outs = [ad.finish_step() for ad in ads]
            flat = [(m.download(ad.grads), m.download(ad.p_on.detach() if hasattr(ad.p_on, "detach") else ad.p_on)) for ad in ads]
            for r in range(1, world):
                assert np.array_equal(flat[0][0].view(np.uint32), flat[r][0].view(np.uint32)), "%s step %d: gradients of replica %d differ" % (what, k, r)
                assert np.array_equal(flat[0][1].view(np.uint32), flat[r][1].view(np.uint32)), "%s step %d: parameters of replica %d differ" % (what, k, r)
                assert outs[0]["grad_norm"] == outs[r]["grad_norm"], "%s step %d: norm of replica %d differs" % (what, k, r)
            o = oracle.step(k, conv_masks=masks)
            print("%s step %d: hidden ReLU margin %.3e (min over %d ranks)" % (what, k, o["margin"], world))
            assert o["margin"] >= RELU_MARGIN, \
                "%s: ill-conditioned seed at step %d: a hidden pre-activation within rounding noise of 0 (%.3e; " \
                "tools/ladder_seeds.py --exchange)" % (what, k, o["margin"])
            for r, pr in enumerate(o["per_rank"]):
                print("%s step %d rank %d: conv ReLU decisions that differ from the oracle's own, per layer (count, largest |pre|, "
                      "largest |pre| / bound): %s" % (what, k, r, ["%d %.1e %.1e" % f for f in pr["conv_flips"]]))
                assert all(ratio < 1.0 for _n, _a, ratio in pr["conv_flips"]), \
                    "%s step %d rank %d: a conv ReLU decision differs outside its rounding bound: %s" % (what, k, r, pr["conv_flips"])
                got_t["s%d_r%d_loss" % (k, r)], want_t["s%d_r%d_loss" % (k, r)] = outs[r]["loss"], pr["loss"]
            got_t["s%d_grad_norm" % k], want_t["s%d_grad_norm" % k] = np.float32(outs[0]["grad_norm"]), np.float32(o["total"])
            for name in o["clipped"]:
                got_t["s%d_grad/%s" % (k, name)], want_t["s%d_grad/%s" % (k, name)] = outs[0]["grads"][name], o["clipped"][name]
            for name, p in ads[0].params().items():
                got_t["s%d_param/%s" % (k, name)], want_t["s%d_param/%s" % (k, name)] = p, o["params"][name]
        assert_learn_trace_matches(got_t, want_t, label=what)
    finally:
        for ad in ads:
            lib.rb_learner_set_exchange(ad.h, 1, None, None)
            ad.close()


# =============================================================================== seed search (CPU, oracle only)
def oracle_margins(case, seed):
    """The oracle's hidden_relu_margin of both steps of `seed`, the smallest over the ranks (step 1 on its own post-Adam
    parameters of step 0)."""
    run = MeanOracle(learn_inputs(case_config(case), LEARN_CASES[case].world, seed))
    return tuple(run.step(k)["margin"] for k in range(2))


def find_seed(case, n=14):
    """-> (found, seen).  found = (seed, margins) of the first seed in [0, n) whose margins are all at least SPARE x RELU_MARGIN, or
    None: the row then has to be masked.  seen: every seed tried."""
    seen = []
    for seed in range(n):
        seen.append((seed, oracle_margins(case, seed)))
        if min(seen[-1][1]) >= SPARE * RELU_MARGIN:
            return seen[-1], seen
    return None, seen
