"""Shrink-and-perturb resets (rb_learner_shrink_perturb, csrc/param_reset.h) against tests/reset_oracle.py, BIT for bit.  Shared by
tests/test_param_reset_emu.py (NumpyMem, host interpreter) and tests/test_param_reset_gpu.py (TorchMem).

The nets are the smallest that still cross every branch of k_shrink_perturb:
  de64     data-efficient, hidden 64, atoms 51, actions 3: fc_z_a.bias_* starts 51 floats into its segment, quads straddle tensors
  de48     data-efficient, hidden 48, atoms 2, actions 1: fc_z_v.bias_* and fc_z_a.bias_* are two floats each and share ONE quad
  canon48  canonical, hidden 48, atoms 21, actions 4: three conv layers, 166 workgroups
Parameters, target and moments are filled with distinct non-zero values, the align64 padding included."""
import ctypes as C

import numpy as np

import reset_oracle as RO
from cabi_adapter import learner_config, query_layout
from rainbow_amd import _lib as L

F32 = np.float32
NETS = {
    "de64": dict(architecture="data-efficient", hidden=64, atoms=51, actions=3),
    "de48": dict(architecture="data-efficient", hidden=48, atoms=2, actions=1),
    "canon48": dict(architecture="canonical", hidden=48, atoms=21, actions=4),
}
ALPHAS = ((0.5, 0.0), (0.8, 0.25), (0.0, 0.0), (1.0, 0.0), (1.0, 1.0))
STD = 0.1
SEED, DRAW = 0x1234567890ABCDEF, 2 ** 32 + 5       # (both above 32 bits: every key and counter word is in use)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _store(buf, arr):
    if isinstance(buf, np.ndarray):
        buf[...] = arr
    else:
        import torch
        buf.copy_(torch.from_numpy(np.ascontiguousarray(arr)))


class Rig:
    def __init__(self, lib, Mem, net, learner_seed=1234):
        self.lib, self.mem = lib, Mem()
        m = self.mem
        c = dict(NETS[net], batch=4, multi_step=3, discount=0.99, history=4, v_min=-10.0, v_max=10.0)
        self.cfg = learner_config(c)
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

    def close(self):
        if self.h:
            self.lib.rb_learner_destroy(self.h)
            self.h = None

    def fill(self, seed):
        """Distinct non-zero values everywhere, padding included: |x| in [0.25, 1.75) for p, t, m, g; v in [1e-4, 2e-4)."""
        rs = np.random.RandomState(seed)
        st = {}
        for k in "ptmg":
            st[k] = (np.where(rs.rand(self.n) < 0.5, -1.0, 1.0) * (0.25 + 1.5 * rs.rand(self.n))).astype(F32)
        st["v"] = (1e-4 * (1.0 + rs.rand(self.n))).astype(F32)
        self.load(st)
        return st

    def load(self, st):
        for k, a in st.items():
            _store(self.bufs[k], a)
        self.mem.sync()

    def state(self):
        self.mem.sync()
        return {k: np.array(self.mem.download(b), copy=True) for k, b in self.bufs.items()}

    def reset(self, a_enc, a_head, seed=SEED, draw=DRAW, with_target=1, moments=True, std=STD):
        m, b = self.mem, self.bufs
        return self.lib.rb_learner_shrink_perturb(self.h, a_enc, a_head, std, seed, draw, with_target,
                                                  m.ptr(b["m"]) if moments else None, m.ptr(b["v"]) if moments else None, m.stream)


def same(got, want, label, keys="ptmvg"):
    for k in keys:
        bad = _bits(got[k]) != _bits(want[k])
        assert not bad.any(), (label, k, int(bad.sum()), int(np.argmax(bad)))


def oracle_check(lib, Mem, net):
    """Online, target and both moments equal the oracle bit for bit for every pair of ALPHAS; tensors with alpha = 1 and every padding
    element are byte-identical to before; (1, 1) changes nothing at all; the gradient is never touched."""
    rig = Rig(lib, Mem, net)
    _, covered = RO.phi_flat(rig.layout, rig.n, STD, SEED, DRAW)
    assert 0 < int((~covered).sum()) and covered[0]
    for k, (ae, ah) in enumerate(ALPHAS):
        st = rig.fill(10 + k)
        L.check(lib, rig.reset(ae, ah))
        got = rig.state()
        want, touched = RO.shrink_perturb(rig.layout, st, ae, ah, STD, SEED, DRAW)
        want["g"] = st["g"]
        assert not (touched & ~covered).any()
        same(got, want, (net, ae, ah))
        for key in "ptmv":
            assert np.array_equal(_bits(got[key][~touched]), _bits(st[key][~touched])), (net, ae, ah, key, "alpha = 1 tensors and padding")
            if touched.any():
                assert not np.array_equal(_bits(got[key][touched]), _bits(st[key][touched])), (net, ae, ah, key, "nothing moved")
        if (ae, ah) == (1.0, 1.0):
            same(got, st, (net, "(1, 1) must change nothing"))
        else:
            assert touched.any()
    rig.close()


def bad_inputs_check(lib, Mem, net):
    """alpha = 0 never reads theta: NaN and inf planted in the online and the target parameters (first and last element of every
    tensor, and one element in eight elsewhere) do not survive, and online equals target bitwise on every tensor."""
    rig = Rig(lib, Mem, net)
    st = rig.fill(31)
    _, covered = RO.phi_flat(rig.layout, rig.n, STD, SEED, DRAW)
    rs = np.random.RandomState(5)
    for k, bad in (("p", np.nan), ("t", np.inf)):
        plant = covered & (rs.rand(rig.n) < 0.125)
        for off, shape in rig.layout.values():
            plant[off] = plant[off + int(np.prod(shape)) - 1] = True
        st[k][plant] = bad
        st[k][plant & (rs.rand(rig.n) < 0.5)] = -np.inf if k == "p" else np.nan
    rig.load(st)
    L.check(lib, rig.reset(0.0, 0.0))
    got = rig.state()
    assert np.isfinite(got["p"][covered]).all() and np.isfinite(got["t"][covered]).all()
    assert np.array_equal(_bits(got["p"][covered]), _bits(got["t"][covered]))
    want, _ = RO.shrink_perturb(rig.layout, st, 0.0, 0.0, STD, SEED, DRAW)
    same(got, want, (net, "alpha = 0 with non-finite inputs"), keys="ptmv")
    rig.close()


def target_off_check(lib, Mem, net):
    """with_target = 0 leaves the target alone; NULL moments leave the moments alone; nothing else differs."""
    rig = Rig(lib, Mem, net)
    for wt, mom in ((0, True), (1, False), (0, False)):
        st = rig.fill(40 + 2 * wt + int(mom))
        L.check(lib, rig.reset(0.5, 0.0, with_target=wt, moments=mom))
        got = rig.state()
        want, _ = RO.shrink_perturb(rig.layout, st, 0.5, 0.0, STD, SEED, DRAW, with_target=bool(wt), moments=mom)
        want["g"] = st["g"]
        same(got, want, (net, "with_target", wt, "moments", mom))
        if not wt:
            assert np.array_equal(_bits(got["t"]), _bits(st["t"]))
        if not mom:
            assert np.array_equal(_bits(got["m"]), _bits(st["m"])) and np.array_equal(_bits(got["v"]), _bits(st["v"]))
    rig.close()


def keys_check(lib, Mem, net):
    """Two draws give different phi; the same (seed, draw) on two handles created with different learner seeds gives the same phi
    (replicas); another seed gives another phi."""
    a, b = Rig(lib, Mem, net, learner_seed=1), Rig(lib, Mem, net, learner_seed=99)
    uniform = np.zeros(a.n, bool)
    for off, numel, uni, _v, _e in RO.tensor_rules(a.layout, STD).values():
        uniform[off:off + numel] = uni
    phis = {}
    for tag, rig, seed, draw in (("a0", a, 7, 0), ("a1", a, 7, 1), ("b0", b, 7, 0), ("s8", b, 8, 0)):
        rig.fill(3)
        L.check(lib, rig.reset(0.0, 0.0, seed=seed, draw=draw))
        phis[tag] = rig.state()["p"]
        want, _ = RO.phi_flat(rig.layout, rig.n, STD, seed, draw)
        assert np.array_equal(_bits(phis[tag][uniform]), _bits(want[uniform])), tag
    assert np.array_equal(_bits(phis["a0"]), _bits(phis["b0"])), "the learner's own seed must not enter the draw"
    for other in ("a1", "s8"):
        assert float(np.mean(phis["a0"][uniform] != phis[other][uniform])) > 0.99, other
    a.close(); b.close()


def largest_uniform_tensor(layout):
    name = max((k for k in layout if k.startswith("convs") or k.endswith("_mu")), key=lambda k: int(np.prod(layout[k][1])))
    off, shape = layout[name]
    return name, off, int(np.prod(shape))


def in_bands(x, bound, label):
    """A sample of U(-bound, bound): every |x| <= bound; |mean| <= 6 sigma of the mean = 6 bound / sqrt(3 n); the sample variance of
    a uniform has standard deviation sqrt(4 / 5 n) = 0.894 / sqrt(n) relative to bound^2 / 3: a 6 sigma band again."""
    x = np.asarray(x, dtype=np.float64)
    n, b = x.size, float(bound)
    assert np.all(np.abs(x) <= b), (label, "beyond the bound", float(np.max(np.abs(x))), b)
    assert abs(x.mean()) <= 6.0 * b / np.sqrt(3.0 * n), (label, "mean", x.mean())
    assert abs(x.var() / (b * b / 3.0) - 1.0) <= 6.0 * 0.894 / np.sqrt(n), (label, "variance", x.var() / (b * b / 3.0))


def distribution_check(lib, Mem, net):
    """The largest drawn tensor of the net (the oracle already pins every bit of all of them)."""
    rig = Rig(lib, Mem, net)
    rig.fill(2)
    L.check(lib, rig.reset(0.0, 0.0))
    name, off, numel = largest_uniform_tensor(rig.layout)
    bound = RO.tensor_rules(rig.layout, STD)[name][3]
    in_bands(rig.state()["p"][off:off + numel], bound, (net, name))
    rig.close()


def invalid_args_check(lib, Mem, net="de48"):
    rig = Rig(lib, Mem, net)
    st = rig.fill(1)
    for bad in (-0.1, 1.5, float("nan")):
        for which, (ae, ah) in (("alpha_encoder", (bad, 0.5)), ("alpha_head", (0.5, bad))):
            assert rig.reset(ae, ah) == -1, (which, bad)                 # RB_ERR_INVALID
            assert which.encode() in lib.rb_last_error(), lib.rb_last_error()
    same(rig.state(), st, "a refused call must change nothing")
    for ok in ((0.0, 1.0), (1.0, 0.0)):
        L.check(lib, rig.reset(*ok))
    rig.close()
