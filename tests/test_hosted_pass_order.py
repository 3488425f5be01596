"""The hosted optimiser pass (adam_body.h: rb_adam_hosted_block / rb_adam_hosted_pairs) after its loads were reordered into ONE
memory trip per workgroup: status word, step number, norm partials, noise factors and data quads are all requested before the
first wait, and the status branch sits behind the partial sum.  Every test runs on the host interpreter and again on the GPU.

Reference: k_clip_adam by value (adam_kernels.h), which the reordering does not touch.  The hosted and pending forms must equal
it BIT FOR BIT in p, m, v, the stored gradient and the norm — same arithmetic, same summation order — so there is no tolerance.

Shapes.  The learner's own flat buffers are padded to whole quads and are never shorter than a block, so the shapes that can
break a load order are driven through rb_debug_adam_pass (optimizer_host.h; tests only) on synthetic buffers:
  n % 4 != 0 (the tail elements of the last plain block), fewer quads than one block (every load of the upper unroll steps
  clamped), a hole inside a plain block, a pair range that is no multiple of the 512 quads of a pair workgroup;
  1, 255, 256, 257, 4096 and 4097 norm partials: below, at and above one partial per thread, and at and above the 16 per thread
  that are requested in front of the data quads (the 4097th takes the second trip of the partial loop);
  a clip that bites and one that is idle; a failed-draw status: nothing may move and the norm is 0.
The small learner layouts (`dataeff` and its 25-window twin; `implicit_small=1` for the pairs) run through the rigs of
tests/optimizer_scenarios.py: hosted by the sampler launch, as a launch of its own, and flushed."""
import ctypes as C
import math

import numpy as np
import pytest

import optimizer_scenarios as S
import scenarios
from rainbow_amd import _lib as L

F32 = np.float32


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    if request.param == "emu":
        from cabi_adapter import NumpyMem as Mem
        from hipemu import loader
        lib = loader.load()
    else:
        from cabi_adapter import TorchMem as Mem
        lib = L.load()
    vp = C.c_void_p
    lib.rb_debug_adam_pass.restype = C.c_int
    lib.rb_debug_adam_pass.argtypes = [C.c_int32, vp, vp, vp, vp, C.c_int64, vp, C.c_int32, C.c_float, vp, vp, C.c_int64,
                                       C.c_double, C.c_double, C.c_double, C.c_double, vp, C.c_int64, C.c_int64, C.c_int32,
                                       C.c_int32, vp, vp, vp, vp, vp]
    return lib, Mem


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def run_pass(lib, mem, form, st, parts, max_norm, step, status, pair=None):
    """One pass over uploaded copies of st's p, g, m, v.  -> (p, g, m, v after, norm, the pair pass's clipped word)."""
    n = st["p"].size
    dev = {k: mem.upload(st[k]) for k in "pgmv"}
    part, norm = mem.upload(np.asarray(parts, F32)), mem.upload(np.full(1, -1.0, F32))
    ctr, stat = mem.upload(np.array([step], np.int64)), mem.upload(np.array([status, 0, 0, 0], np.int32))
    clipped, args = mem.upload(np.full(4, -1, np.int32)), mem.upload(np.zeros(32, np.int64))
    pr = [0, 0, 0, 0, None, None, None]
    keep = []
    if pair is not None and form == 1:
        keep = [mem.upload(pair["eout"]), mem.upload(pair["ein"])]
        pr = [pair["mu4"], pair["len4"], pair["f4"], pair["split_row"], mem.ptr(keep[0]), mem.ptr(keep[1]), mem.ptr(clipped)]
    L.check(lib, lib.rb_debug_adam_pass(form, mem.ptr(dev["p"]), mem.ptr(dev["g"]), mem.ptr(dev["m"]), mem.ptr(dev["v"]), n,
                                       mem.ptr(part), len(parts), max_norm, mem.ptr(norm), mem.ptr(ctr), step, S.LR, S.B1, S.B2,
                                       S.EPS, mem.ptr(stat), *pr, mem.ptr(args), mem.stream))
    mem.sync()
    out = {k: np.array(mem.download(dev[k]), copy=True) for k in "pgmv"}
    return out, F32(mem.download(norm)[0]), int(mem.download(clipped)[0])


def make_state(n, seed):
    rs = np.random.RandomState(seed)
    return dict(p=rs.randn(n).astype(F32), g=(1e-2 * rs.randn(n)).astype(F32), m=(1e-3 * rs.randn(n)).astype(F32),
                v=(1e-4 * rs.rand(n)).astype(F32))


def make_parts(count, seed):
    return (np.random.RandomState(seed).rand(count) + 0.01).astype(F32)


def max_norm_for(parts, bite):
    return float(F32((0.3 if bite else 3.0) * math.sqrt(float(np.sum(parts.astype(np.float64))))))


def pair_sigma(st, pair):
    """g with the sigma quads replaced by fl32(g_mu * fl32(eps_out[row] * eps_in[col])): the pair pass's own expression."""
    rows, cols = pair["len4"] // pair["f4"], 4 * pair["f4"]
    mu, sg = 4 * pair["mu4"], 4 * (pair["mu4"] + pair["len4"])
    second = (np.arange(rows) >= pair["split_row"]).astype(np.int64)
    prod = (pair["eout"][:, None] * pair["ein"].reshape(2, cols)[second]).astype(F32)
    g = st["g"].copy()
    g[sg:sg + rows * cols] = (g[mu:mu + rows * cols].reshape(rows, cols) * prod).astype(F32).ravel()
    return g, (sg, sg + rows * cols)


def same(a, b, label, keys="pgmv"):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (label, k, int(np.sum(_bits(a[k]) != _bits(b[k]))))


# n (floats), seed: fewer quads than one block of 1024 with a 3-element tail; three blocks with a 1-element tail
PLAIN_SHAPES = ((4 * 700 + 3, 1), (4 * (2 * 1024 + 37) + 1, 2))
PART_COUNTS = (1, 255, 256, 257, 4096, 4097)


@pytest.mark.parametrize("n,seed", PLAIN_SHAPES)
def test_plain_pass_equals_clip_adam_by_value(backend, n, seed):
    lib, Mem = backend
    mem = Mem()
    st = make_state(n, seed)
    for ci, count in enumerate(PART_COUNTS):
        parts = make_parts(count, 10 * seed + ci)
        bite = ci % 2 == 0
        step = (1, 7, 2 ** 32 + 3)[ci % 3]
        mx = max_norm_for(parts, bite)
        ref, rnorm, _ = run_pass(lib, mem, 0, st, parts, mx, step, 0)
        got, gnorm, _ = run_pass(lib, mem, 1, st, parts, mx, step, 0)
        label = "n %d / %d partials / bite %s / step %d" % (n, count, bite, step)
        assert float(rnorm) > 0 and (float(rnorm) > mx) == bite, label
        assert np.array_equal(_bits(ref["g"]), _bits(st["g"])) != bite, (label, "the stored gradient follows the clip")
        assert not np.array_equal(_bits(ref["p"]), _bits(st["p"])), label
        assert _bits(gnorm) == _bits(rnorm), (label, "norm", float(gnorm), float(rnorm))
        same(ref, got, label)


def pair_case():
    """Three plain blocks around a hole that starts inside the second one; 1083 = 19 x 57 pair quads = two whole pair
    workgroups and one of 59 quads; rows from 30 on take eps_in from the second vector; a 2-element tail."""
    pair = dict(mu4=1500, len4=1083, f4=19, split_row=30)
    n = 4 * (1500 + 2 * 1083 + 700) + 2
    rs = np.random.RandomState(5)
    pair["eout"] = rs.randn(57).astype(F32)
    pair["ein"] = rs.randn(2 * 4 * 19).astype(F32)
    return n, pair


@pytest.mark.parametrize("bite", (True, False))
def test_pair_pass_equals_clip_adam_by_value_on_the_materialised_gradient(backend, bite):
    lib, Mem = backend
    mem = Mem()
    n, pair = pair_case()
    st = make_state(n, 3)
    g_full, (slo, shi) = pair_sigma(st, pair)
    st["g"][slo:shi] = 123.0                     # the pair pass never reads the sigma gradient: a sentinel, not the product
    parts = make_parts(300, 31)
    mx = max_norm_for(parts, bite)
    ref, rnorm, _ = run_pass(lib, mem, 0, dict(st, g=g_full), parts, mx, 5, 0)
    got, gnorm, clipped = run_pass(lib, mem, 1, st, parts, mx, 5, 0, pair)
    assert (float(rnorm) > mx) == bite and _bits(gnorm) == _bits(rnorm)
    assert clipped == (1 if bite else 0)
    same(ref, got, ("pairs", bite), keys="pmv")
    if bite:                                     # the scaled gradients are stored back, sigma's included
        assert np.array_equal(_bits(got["g"]), _bits(ref["g"]))
    else:                                        # nothing is stored: the sentinel is still there
        assert np.array_equal(_bits(got["g"]), _bits(st["g"])) and np.array_equal(_bits(ref["g"]), _bits(g_full))


@pytest.mark.parametrize("with_pairs", (False, True))
def test_failed_draw_status_moves_nothing_and_reports_norm_zero(backend, with_pairs):
    lib, Mem = backend
    mem = Mem()
    n, pair = pair_case()
    st = make_state(n, 4)
    parts = make_parts(4097, 41)
    for form in ((1,) if with_pairs else (0, 1)):
        got, norm, clipped = run_pass(lib, mem, form, st, parts, max_norm_for(parts, True), 9, 1, pair if with_pairs else None)
        same(st, got, ("failed draw", form, with_pairs))
        assert float(norm) == 0.0 and _bits(norm) == 0
        assert clipped == -1, "a skipped pair pass stores no clip decision"


def test_hosted_flushed_and_pending_forms_on_the_small_layouts(backend, monkeypatch):
    """dataeff and its 25-window twin through the rigs: k_clip_adam by value and by device counter, flush (k_adam_pending), hosted
    by the sampler launch (k_sample), the pending pass as a launch of its own behind the 25-transition window — every form against
    the float64 reference and bit-identical to the others, for a clip that bites and an idle one."""
    lib, Mem = backend
    cases = (("scales", "bite", 3), ("zeros", "idle", 2 ** 32 + 3))
    assert S.form_group_check(lib, Mem, monkeypatch, cases=cases) == {3, 2 ** 32 + 3}


def _squares_with_root(norm):
    """One partial x with sqrtf(x) == norm exactly (float32 sqrt maps two binades onto one: a preimage exists)."""
    x = F32(norm) * F32(norm)
    for _ in range(8):
        r = np.sqrt(x, dtype=F32)
        if r == F32(norm):
            return x
        x = np.nextafter(x, F32(np.inf) if r < norm else F32(0), dtype=F32)
    raise AssertionError("no float32 square root preimage of %r" % norm)


def test_pair_workgroups_of_the_small_layout_equal_clip_adam_by_value(backend, monkeypatch):
    """A real train step under DEFER_UPDATE | IMPLICIT_SIGMA (implicit_small=1) leaves the pair pass pending; it then runs flushed
    (k_adam_pending) or hosted (k_sample).  Reference: k_clip_adam by value over the state downloaded in front of the pass, the
    sigma gradient materialised on the host, one partial whose square root IS the norm the device reported (same coefficient)."""
    from cabi_adapter import query_layout
    from ts_scenarios import ts_args
    lib, Mem = backend
    name, flags = "dataeff", L.LEARNER_DEFER_UPDATE | L.LEARNER_IMPLICIT_SIGMA
    monkeypatch.setenv("RB_OPTS", "implicit_small=1,spec_draw=0")
    assert S.plan_reports_implicit_sigma(lib, name, "implicit_small=1,spec_draw=0", flags)
    rig = S.build_rig(lib, Mem, name, True, flags)
    m, ad = rig.mem, rig.ad
    nl = query_layout(lib, ad.cfg, lib.rb_learner_noise_layout)
    B = scenarios.LEARN_CONFIGS[name]["batch"]
    for rnd, (how, max_norm) in enumerate((("hosted", 1e-3), ("hosted", 10.0), ("flush", 1e-3))):
        ts = ts_args(name, m, rig.rp, ad, rig.out, rig.job, 0.4, 0, max_norm)
        ts.norm_dev = m.ptr(rig.norm)
        L.check(lib, lib.rb_learner_train_step(ad.h, C.byref(ts), m.stream))
        before = S.state(rig)
        g_full = S.sigma_product(ad, before["g"], S._dl(m, ad.z_on), nl)
        step = int(S._dl(m, rig.ctr)[0])
        assert step == rnd + 1
        job2 = L.NoiseJob()
        L.check(lib, lib.rb_learner_noise_job(ad.h, 2, C.byref(job2)))
        if how == "flush":
            L.check(lib, lib.rb_learner_flush(ad.h, m.stream))
        else:
            job_out = L.NoiseJob()
            assert lib.rb_learner_attach_pending(ad.h, C.byref(job2), B, C.byref(job_out)) == 1
            S._sample(rig, job_out)
            L.check(lib, lib.rb_learner_pending_launched(ad.h))
        after = S.state(rig)
        norm = F32(S._dl(m, rig.norm)[0])
        assert (float(norm) > max_norm) == (max_norm < 1.0), (how, max_norm, float(norm))
        ref, rnorm, _ = run_pass(lib, m, 0, dict(before, g=g_full), [_squares_with_root(norm)], max_norm, step, 0)
        assert _bits(rnorm) == _bits(norm)
        same(ref, after, (how, max_norm), keys="pmv")
        if max_norm < 1.0:
            L.check(lib, lib.rb_learner_flush(ad.h, m.stream))       # (materialises nothing: the pass stored the scaled gradients)
            assert np.array_equal(_bits(S.state(rig)["g"]), _bits(ref["g"])), (how, "the stored gradient")
    S.close_rig(rig)
