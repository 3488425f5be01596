"""Oracle of the dormant-unit recycling (ReDo; rb_learner_unit_activity / _dormant_mask / _recycle_units, csrc/unit_recycle.h), numpy
only.  Everything is derived from the (offset, shape) layout of rb_learner_param_layout: no offset is recomputed here.

Units: an output channel of a conv layer, a hidden unit of fc_h_v, of fc_h_a; layers in that order, units numbered in that order.
  activity[i]   float64 sum of the unit's post-ReLU activations over the rows (and positions)
  dormant       activity[i] * N_l <= tau * S_l in float64, S_l the layer's sum (NaN compares false)
  recycle       incoming parameters <- phi; outgoing weight_mu / conv weights <- 0, outgoing weight_sigma <- its constant; an element
                that is both gets the outgoing rule; both Adam moments of every written element <- 0
phi of flat element e: word e & 3 of Philox4x32-10(key = seed ^ TAG, counter hi = draw, lo = e >> 2), u = f32(x >> 8) * 2^-24,
phi = bound * (2u - 1) in float32, or the tensor's constant (the sigma tensors); bounds and constants are reset_oracle.tensor_rules'."""
import numpy as np

import reset_oracle as RO

F32 = np.float32
TAG = 0x5245444F                         # "REDO" (RB_REDO_KEY_TAG)
M64 = (1 << 64) - 1
HIDDEN = ("fc_h_v", "fc_h_a")
UNTOUCHED, INCOMING, OUTGOING = 0, 1, 2


def conv_names(layout):
    return sorted((k for k in layout if k.startswith("convs") and k.endswith(".weight")), key=lambda k: int(k.split(".")[1]))


def unit_layout(layout):
    """[(layer name, units)] in the order of rb_learner_unit_layout."""
    out = [(name.rsplit(".", 1)[0], layout[name][1][0]) for name in conv_names(layout)]
    return out + [(s, layout[s + ".weight_mu"][1][0]) for s in HIDDEN]


def firsts(layout):
    units = [n for _, n in unit_layout(layout)]
    return np.concatenate([[0], np.cumsum(units)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ activity --
def per_unit(conv_acts, h):
    """conv_acts: [B, cout, oh, ow] per conv layer, h: [B, 2H] -> per unit: the float64 sum, the float64 sum of |.| and the number
    of terms."""
    s, a, n = [], [], []
    for x in list(conv_acts) + [np.asarray(h)[:, :, None]]:
        x = np.asarray(x, dtype=np.float64)
        x = x.reshape(x.shape[0], x.shape[1], -1)
        s.append(x.sum(axis=(0, 2))); a.append(np.abs(x).sum(axis=(0, 2))); n.append(np.full(x.shape[1], x.shape[0] * x.shape[2]))
    return np.concatenate(s), np.concatenate(a), np.concatenate(n)


# ---------------------------------------------------------------------------------------------------------------- mask --
def dormant(layout, activity, tau):
    """-> (mask uint8 [U], counts int32 [n_layers], scores float64 [U]: activity * N / S, 0 where S == 0)."""
    act = np.asarray(activity, dtype=np.float64)
    f = firsts(layout)
    mask, scores, counts = np.zeros(act.size, np.uint8), np.zeros(act.size, np.float64), np.zeros(len(f) - 1, np.int32)
    with np.errstate(all="ignore"):
        for k in range(len(f) - 1):
            a = act[f[k]:f[k + 1]]
            n, S = float(a.size), float(a.sum())            # (the tests plant whole numbers: every summation order is exact)
            d = a * n <= np.float64(tau) * S                # NaN: False
            mask[f[k]:f[k + 1]] = d
            counts[k] = int(d.sum())
            scores[f[k]:f[k + 1]] = 0.0 if S == 0.0 else a * n / S
    return mask, counts, scores


# ------------------------------------------------------------------------------------------------------------- recycle --
def phi_flat(layout, n_params, noisy_std, seed, draw):
    """phi of every element that belongs to a tensor, float32 [n_params]."""
    assert n_params % 4 == 0
    x = RO.philox4x32_10((int(seed) & M64) ^ TAG, int(draw) & M64, np.arange(n_params // 4, dtype=np.uint64)).reshape(-1)
    u = (x >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
    r = (F32(2.0) * u - F32(1.0)).astype(F32)
    phi = np.zeros(n_params, F32)
    for name, (off, numel, uniform, val, _enc) in RO.tensor_rules(layout, noisy_std).items():
        phi[off:off + numel] = (val * r[off:off + numel]).astype(F32) if uniform else val
    return phi


def index_sets(layout, unit):
    """(incoming, outgoing to zero, outgoing to the sigma constant) flat indices of unit `unit`."""
    f = firsts(layout)
    k = int(np.searchsorted(f, unit, side="right")) - 1
    i = int(unit - f[k])
    convs = conv_names(layout)
    empty = np.zeros(0, np.int64)
    if k < len(convs):
        off, (cout, cin, ks, _) = layout[convs[k]]
        K = cin * ks * ks
        inc = np.concatenate([off + i * K + np.arange(K), [layout[convs[k].replace("weight", "bias")][0] + i]])
        if k + 1 < len(convs):
            noff, (ncout, ncin, nks, _) = layout[convs[k + 1]]
            assert ncin == cout
            out0 = (noff + np.arange(ncout)[:, None] * (ncin * nks * nks) + i * nks * nks + np.arange(nks * nks)[None, :]).reshape(-1)
            return inc, out0, empty
        out0, outc = [], []
        for s in HIDDEN:
            moff, (H, F) = layout[s + ".weight_mu"]
            P = F // cout
            assert P * cout == F
            cols = (np.arange(H)[:, None] * F + i * P + np.arange(P)[None, :]).reshape(-1)
            out0.append(moff + cols); outc.append(layout[s + ".weight_sigma"][0] + cols)
        return inc, np.concatenate(out0), np.concatenate(outc)
    s = HIDDEN[k - len(convs)]
    _, (H, F) = layout[s + ".weight_mu"]
    inc = np.concatenate([layout[s + ".weight_mu"][0] + i * F + np.arange(F), layout[s + ".weight_sigma"][0] + i * F + np.arange(F),
                          [layout[s + ".bias_mu"][0] + i, layout[s + ".bias_sigma"][0] + i]])
    z = s.replace("fc_h", "fc_z")
    _, (rows, H2) = layout[z + ".weight_mu"]
    assert H2 == H
    col = np.arange(rows) * H + i
    return inc, layout[z + ".weight_mu"][0] + col, layout[z + ".weight_sigma"][0] + col


def recycle(layout, st, mask, noisy_std, seed, draw, with_target=True, moments=True):
    """st = dict(p, t, m, v) of float32 [n_params] -> (the same after the recycle, kind int8 [n_params]: UNTOUCHED / INCOMING /
    OUTGOING, the number of elements that are incoming to one dormant unit and outgoing from another)."""
    n = st["p"].size
    phi = phi_flat(layout, n, noisy_std, seed, draw)
    rules = RO.tensor_rules(layout, noisy_std)
    const = np.zeros(n, F32)
    for name, (off, numel, uniform, val, _enc) in rules.items():
        if not uniform:
            const[off:off + numel] = val
    kind, val = np.zeros(n, np.int8), np.zeros(n, F32)
    sets = [index_sets(layout, u) for u in np.flatnonzero(np.asarray(mask))]
    for inc, _o0, _oc in sets:
        kind[inc] = INCOMING; val[inc] = phi[inc]
    both = 0
    for _inc, o0, oc in sets:                       # the outgoing rule afterwards: it wins
        both += int((kind[o0] == INCOMING).sum()) + int((kind[oc] == INCOMING).sum())
        kind[o0] = OUTGOING; val[o0] = 0.0
        kind[oc] = OUTGOING; val[oc] = const[oc]
    out = {k: np.array(x, dtype=F32, copy=True) for k, x in st.items()}
    w = kind != UNTOUCHED
    for k in ("p", "t") if with_target else ("p",):
        out[k][w] = val[w]
    if moments:
        out["m"][w] = 0.0
        out["v"][w] = 0.0
    return out, kind, both
