"""Oracle of the shrink-and-perturb reset (rb_learner_shrink_perturb, csrc/param_reset.h), numpy only.

    theta <- alpha * theta + (1 - alpha) * phi            per named tensor of the flat parameter layout
phi of flat element i: word i & 3 of Philox4x32-10(key = seed ^ TAG, counter hi = draw, lo = i >> 2), u = f32(x >> 8) * 2^-24,
r = 2u - 1, phi = bound * r — or the tensor's constant (the sigma tensors).  Everything in float32 in the kernel's operation
order: two products and one sum, om = f32(1) - f32(alpha); alpha == 0 gives phi itself, alpha == 1 leaves the tensor alone.
The distributions are those of rainbow_amd.agent.init_parameters_flat (model.py:25-30, Conv2d's default)."""
import math

import numpy as np

F32 = np.float32
TAG = 0x5245534554                       # "RESET" (RB_RESET_KEY_TAG)
M32 = np.uint64(0xFFFFFFFF)
M64 = (1 << 64) - 1


def philox4x32_10(seed, ctr_hi, ctr_lo):
    """Vectorised over ctr_lo (uint64 array); seed and ctr_hi are Python ints.  -> uint32 [len, 4].  (rb_philox, csrc/rb_common.h)"""
    lo = np.asarray(ctr_lo, dtype=np.uint64)
    c0, c1 = lo & M32, lo >> np.uint64(32)
    c2 = np.full_like(lo, int(ctr_hi) & 0xFFFFFFFF)
    c3 = np.full_like(lo, (int(ctr_hi) >> 32) & 0xFFFFFFFF)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    m0, m1, s32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                                        # 32 x 32 -> 64 bits: no wrap
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0)) & M32, p1 & M32, ((p0 >> s32) ^ c3 ^ np.uint64(k1)) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def symmetric_uniform(seed, draw, n):
    """r = 2u - 1 in float32 for the flat elements 0 .. n - 1 (n a multiple of 4)."""
    assert n % 4 == 0
    x = philox4x32_10((int(seed) & M64) ^ TAG, int(draw) & M64, np.arange(n // 4, dtype=np.uint64)).reshape(-1)
    u = (x >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
    return (F32(2.0) * u - F32(1.0)).astype(F32)


def tensor_rules(layout, noisy_std):
    """{name: (offset, numel, uniform, f32 bound or constant, is_encoder)} from the (offset, shape) layout of
    rb_learner_param_layout.  noisy_std crosses the C ABI as a float32."""
    std = float(F32(noisy_std))
    out = {}
    for name, (off, shape) in layout.items():
        numel = int(np.prod(shape))
        if name.startswith("convs"):
            wshape = layout[name.rsplit(".", 1)[0] + ".weight"][1]
            out[name] = (off, numel, True, F32(1.0 / math.sqrt(int(np.prod(wshape[1:])))), True)
            continue
        layer, kind = name.split(".")
        out_f, in_f = layout[layer + ".weight_mu"][1]
        if kind in ("weight_mu", "bias_mu"):
            out[name] = (off, numel, True, F32(1.0 / math.sqrt(in_f)), False)
        elif kind == "weight_sigma":
            out[name] = (off, numel, False, F32(std / math.sqrt(in_f)), False)
        else:
            out[name] = (off, numel, False, F32(std / math.sqrt(out_f)), False)
    return out


def phi_flat(layout, n_params, noisy_std, seed, draw):
    """phi for every element that belongs to a tensor (float32 [n_params]) and the mask of those elements."""
    r = symmetric_uniform(seed, draw, n_params)
    phi, covered = np.zeros(n_params, F32), np.zeros(n_params, bool)
    for name, (off, numel, uniform, val, _enc) in tensor_rules(layout, noisy_std).items():
        phi[off:off + numel] = (val * r[off:off + numel]).astype(F32) if uniform else val
        covered[off:off + numel] = True
    return phi, covered


def shrink_perturb(layout, st, alpha_encoder, alpha_head, noisy_std, seed, draw, with_target=True, moments=True):
    """st = dict(p, t, m, v) of float32 [n_params] -> the same after the reset, and the mask of the elements it touched."""
    n = st["p"].size
    phi, _ = phi_flat(layout, n, noisy_std, seed, draw)
    out = {k: np.array(x, dtype=F32, copy=True) for k, x in st.items()}
    touched = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for name, (off, numel, _u, _v, enc) in tensor_rules(layout, noisy_std).items():
            a = F32(alpha_encoder if enc else alpha_head)
            if not a < 1.0:
                continue
            om = F32(1.0) - a
            sl = slice(off, off + numel)
            touched[sl] = True
            for k in ("p", "t") if with_target else ("p",):
                out[k][sl] = phi[sl] if a == 0.0 else ((a * st[k][sl]).astype(F32) + (om * phi[sl]).astype(F32)).astype(F32)
            if moments:
                out["m"][sl] = 0.0
                out["v"][sl] = 0.0
    return out, touched
