"""Feature rank and per-tensor norms (rb_learner_features, rb_gram_f64, rb_learner_tensor_norms: csrc/feature_gram.h and
csrc/tensor_norms.h; rainbow_amd/feature_rank.py).  Shared by tests/test_rank_emu.py (NumpyMem, host interpreter) and
tests/test_rank_gpu.py (TorchMem); tests/rank_guard_run.py runs the same launches between guard bands.

Tolerances.
  Gram    K*[i][j] = math.fsum of the float64 products phi_ik phi_jk.  A product of two float32 is exact in float64, so K* is the exact
          sum rounded once.  |K - K*| <= d 2^-53 sum_k |phi_ik| |phi_jk| holds for ANY order of d float64 additions of exact terms
          (d - 1 roundings of partial sums that never exceed the sum of magnitudes, and one for K* itself).
  bits    symmetry, the top-left block property, the independence of ld and the repeat: exact.
  norms   sum a^2: the squares are exact in float64, `count` additions in any order: (count + 2) 2^-53 sum.  sum (a - b)^2: the
          difference and the square round once each (3 2^-53 relative per term), then count - 1 additions: the same bound.  The
          reference takes the difference and the square in long double (64-bit significand: the difference of two float32 whose
          exponents differ by less than 40 is exact there) and sums with math.fsum.  max |a|: exact.
  norm    sqrt(sum_t grad_sumsq) against the learner's own float32 norm: n_params 2^-24 relative, the any-order bound of a
          float32 sum of n_params non-negative terms (the square root halves it; not used).
  sigma   spectrum_metrics on an exact Gram: 1e-9 absolute against numpy.linalg.svd.  An eigenvalue of K / n carries an absolute
          error of a few 2^-53 lambda_1, so sigma = sqrt(lambda) carries about 1e-16 / (2 sigma): every planted sigma stays at or
          above 1e-4, where that is 5e-13."""
import ctypes as C
import functools
import math

import numpy as np

import diag_scenarios as DS
import optimizer_scenarios as S
import redo_scenarios as RS
from rainbow_amd import _lib as L
from rainbow_amd.feature_rank import spectrum_metrics

F32, F64 = np.float32, np.float64
RB_ERR_INVALID, RB_ERR_STATE = -1, -4
U53 = 2.0 ** -53
HIDDEN, CONV = 0, 1
# (n, d, ld): one row and one column; one exact MFMA block; ragged n and d; three k chunks; d below the MFMA's 4; two tile rows
# with a ragged one; three tile rows (six workgroups, off-diagonal tiles) with d = 8 chunks + 1; the conv width; a long chain
GRAM_SHAPES = ((1, 1, 4), (16, 4, 4), (17, 5, 8), (33, 70, 72), (64, 2, 4), (96, 50, 52), (130, 257, 260), (8, 3136, 3136), (40, 1024, 1024))
BITS_SHAPE = (130, 257, 260)
SPECTRUM_SHAPES = ((33, 70), (96, 50), (64, 2))
PLANTED = (1.0, 0.5, 0.2, 0.05, 0.02, 0.004, 0.002, 0.001)     # then 1e-4 for every further singular value
POISON64 = np.uint64(0xC5C5C5C5C5C5C5C5)                       # (a finite double: an element that was never written stays findable)


def _u64(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


def _u32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# =============================================================================== 1: the Gram matrix
def make_phi(n, d, seed):
    """float32 [n, d]: magnitudes 10^U(-3, 2), random signs."""
    rs = np.random.RandomState(seed)
    return (np.where(rs.rand(n, d) < 0.5, -1.0, 1.0) * 10.0 ** rs.uniform(-3.0, 2.0, size=(n, d))).astype(F32)


def padded(phi, ld):
    """[n + 1, ld] with NaN in the pad columns [d, ld) and in the guard row behind row n - 1."""
    n, d = phi.shape
    out = np.full((n + 1, ld), np.nan, F32)
    out[:n, :d] = phi
    return out


def exact_gram(phi):
    """(K*, A): K*[i][j] = fsum_k of the exact float64 products; A[i][j] = sum_k |phi_ik| |phi_jk| (the bound's scale)."""
    p = np.asarray(phi, dtype=F64)
    n = p.shape[0]
    K = np.empty((n, n), F64)
    for i in range(n):
        for j in range(i, n):
            K[i, j] = K[j, i] = math.fsum(p[i] * p[j])
    a = np.abs(p)
    return K, a @ a.T


@functools.lru_cache(maxsize=None)
def gram_case(n, d):
    phi = make_phi(n, d, 1000 * n + d)
    K, A = exact_gram(phi)
    for x in (phi, K, A):
        x.setflags(write=False)
    return phi, K, A


def run_gram(lib, mem, phi, ld, rows=None, poison=None):
    """rb_gram_f64 on the first `rows` rows of phi laid out at ld -> K float64 [rows, rows]."""
    n, d = phi.shape
    rows = n if rows is None else rows
    pbuf = mem.upload(padded(phi[:rows], ld))
    kbuf = mem.upload(np.full(rows * rows, np.nan if poison is None else poison, F64))
    L.check(lib, lib.rb_gram_f64(mem.ptr(pbuf), rows, d, ld, mem.ptr(kbuf), mem.stream))
    mem.sync()
    return mem.download(kbuf).reshape(rows, rows)


def gram_check(lib, Mem, shape, notes=None):
    """K against the exact reference inside the derived bound, finite and fully written although the pad columns, the guard row and K
    itself start as NaN."""
    n, d, ld = shape
    phi, want, A = gram_case(n, d)
    K = run_gram(lib, Mem(), phi, ld)
    assert np.isfinite(K).all(), (shape, "K must come back finite and fully written", int((~np.isfinite(K)).sum()))
    err, bound = np.abs(K - want), d * U53 * A
    ratio = float((err / bound).max())
    line = "gram (n %d, d %d, ld %d): largest error / bound %.3g" % (n, d, ld, ratio)
    print(line)
    if notes is not None:
        notes.append(line)
    assert np.all(err <= bound), (shape, ratio)


def gram_bits_check(lib, Mem):
    """At (130, 257, 260): K == K^T bit for bit; the K of the first 33, 64 and 65 rows is the top-left block of the full K; ld 260
    and ld 512 give the same bits; two runs are bit-equal."""
    n, d, ld = BITS_SHAPE
    phi = gram_case(n, d)[0]
    mem = Mem()
    K = run_gram(lib, mem, phi, ld)
    assert np.array_equal(_u64(K), _u64(K.T)), "K must be symmetric bit for bit"
    for rows in (33, 64, 65):
        sub = run_gram(lib, mem, phi, ld, rows=rows)
        assert np.array_equal(_u64(sub), _u64(K[:rows, :rows])), "the K of the first %d rows must be the top-left block" % rows
    assert np.array_equal(_u64(run_gram(lib, mem, phi, 512)), _u64(K)), "the result must not depend on ld"
    assert np.array_equal(_u64(run_gram(lib, mem, phi, ld)), _u64(K)), "a repeated run must be bit-identical"


def gram_refusals_check(lib, Mem):
    """Every bound of rb_gram_f64 one step outside it: RB_ERR_INVALID, the argument named, K's poison intact."""
    mem = Mem()
    n, d, ld = 8, 6, 8
    pbuf = mem.upload(np.ones(16 * ld + 8, F32))
    kbuf = mem.upload(np.full(64 + 1, POISON64, np.uint64).view(F64))
    big = mem.empty((4,), np.float32)                                  # (never read: the call is refused before anything is launched)
    p, k = mem.ptr(pbuf), mem.ptr(kbuf)
    cases = [((p, 0, d, ld, k), b"n must"), ((p, 4097, d, 8, k), b"n must"), ((p, n, 0, ld, k), b"d must"),
             ((p, n, d, 4, k), b"ld must be >="), ((p, n, 5, 6, k), b"multiple of 4"), ((p + 4, n, d, ld, k), b"phi_dev"),
             ((p, n, d, ld, k + 4), b"gram_dev"), ((None, n, d, ld, k), b"phi_dev"), ((p, n, d, ld, None), b"gram_dev"),
             ((mem.ptr(big), 4096, 131072, 131072, k), b"2 GiB")]     # 4 * 4096 * 131072 = 2^31: one step outside
    for args, word in cases:
        assert lib.rb_gram_f64(*args, mem.stream) == RB_ERR_INVALID, args[1:4]
        assert word in lib.rb_last_error(), (word, lib.rb_last_error())
    mem.sync()
    assert np.all(mem.download(kbuf).view(np.uint64) == POISON64), "a refused call must leave K alone"
    L.check(lib, lib.rb_gram_f64(p, n, d, ld, k, mem.stream))         # the accepted edge: ld % 4 == 0, ld >= d, aligned
    L.check(lib, lib.rb_gram_f64(mem.ptr(big), 1, 1, 4, k, mem.stream))
    mem.sync()
    assert mem.download(kbuf).view(np.uint64)[64] == POISON64


# =============================================================================== 2: the spectrum
def planted_phi(n, d, seed=0):
    """Phi = sqrt(n) U diag(s) V^T in float64 with orthonormal U [n, r], V [d, r], r = min(n, d), s = PLANTED then 1e-4."""
    r = min(n, d)
    rs = np.random.RandomState(seed + 31 * n + d)
    U = np.linalg.qr(rs.randn(n, r))[0]
    V = np.linalg.qr(rs.randn(d, r))[0]
    s = np.array((PLANTED + (1e-4,) * r)[:r])
    return math.sqrt(n) * (U * s) @ V.T, s


def spectrum_check(n, d):
    """No kernel: spectrum_metrics on the float64 Gram of a planted Phi.  sigma within 1e-9 of numpy.linalg.svd; feature_rank 5 and
    srank 5 (d = 2 caps both at 2): the cumulative shares are 0.98 at k = 4 and 0.99+ at k = 5, the threshold 0.99 sits in a gap."""
    phi, s = planted_phi(n, d)
    m = spectrum_metrics(phi @ phi.T, n, d)
    sv = np.linalg.svd(phi / math.sqrt(n), compute_uv=False)
    r = min(n, d)
    assert m["finite"] and m["singular_values"].shape == (r,)
    err = float(np.abs(m["singular_values"] - sv[:r]).max())
    print("spectrum (n %d, d %d): largest |sigma - svd| %.3g" % (n, d, err))
    assert err <= 1e-9, (n, d, err)
    want = min(5, d)
    assert m["feature_rank"] == want and m["srank"] == want, (n, d, m["feature_rank"], m["srank"])
    share = np.cumsum(sv[:r]) / sv[:r].sum()
    if r >= 5:
        assert share[3] < 0.99 - 1e-3 and share[4] > 0.99 + 1e-3, share[:6]
    p = sv[:r] / sv[:r].sum()
    assert abs(m["effective_rank"] - math.exp(-float((p * np.log(p)).sum()))) <= 1e-6
    assert abs(m["mean_sq_norm"] - float((s ** 2).sum())) <= 1e-9 and abs(m["top_share"] - 1.0 / float((s ** 2).sum())) <= 1e-9


def spectrum_edges_check():
    """A non-finite K never reaches LAPACK; an all-zero K has rank 0; a wrong shape is refused."""
    K = np.eye(4)
    for bad in (np.nan, np.inf):
        Kb = K.copy()
        Kb[1, 2] = bad
        m = spectrum_metrics(Kb, 4, 9)
        assert m["finite"] is False and np.isnan(m["singular_values"]).all() and m["singular_values"].shape == (4,)
        assert all(math.isnan(m[k]) for k in ("feature_rank", "srank", "effective_rank", "mean_sq_norm", "top_share"))
    z = spectrum_metrics(np.zeros((3, 3)), 3, 2)
    assert z["finite"] and z["feature_rank"] == 0 and z["srank"] == 0 and z["effective_rank"] == 0.0 and z["singular_values"].shape == (2,)
    one = spectrum_metrics(4.0 * np.eye(4), 4, 4)                       # sigma = (1, 1, 1, 1)
    assert one["feature_rank"] == 4 and one["srank"] == 4 and abs(one["effective_rank"] - 4.0) < 1e-12 and abs(one["top_share"] - 0.25) < 1e-12
    try:
        spectrum_metrics(np.eye(3), 4, 4)
    except ValueError:
        pass
    else:
        raise AssertionError("a K of the wrong shape must be refused")


def eigenvalues_mp(M, n):
    """The eigenvalues of the float64 matrix M / n to 40 digits, ascending (mpmath: LAPACK's own error, a few 2^-53 lambda_1, is as
    large as the difference the check below is about)."""
    import mpmath
    with mpmath.workdps(40):
        return sorted(mpmath.eigsy(mpmath.matrix(M.tolist()) / n, eigvals_only=True))


@functools.lru_cache(maxsize=None)
def planted_case(n, d):
    phi = planted_phi(n, d)[0].astype(F32)
    want = exact_gram(phi)[0]
    want.setflags(write=False)
    phi.setflags(write=False)
    return phi, want, tuple(eigenvalues_mp(want, n))


def end_to_end_check(lib, Mem, n, d):
    """The planted Phi, rounded to float32, through the device Gram: the eigenvalues of K / n within ||K - K*||_F / n of those of the
    exact K* / n (Weyl; both spectra to 40 digits, so that the inequality is not blurred by the solver), and the two integer ranks
    of the planted matrix from spectrum_metrics on the device's K."""
    phi, want, lam_star = planted_case(n, d)
    ld = (d + 3) // 4 * 4
    K = run_gram(lib, Mem(), phi, ld)
    lam = eigenvalues_mp(K, n)
    err, bound = float(max(abs(a - b) for a, b in zip(lam, lam_star))), float(np.linalg.norm(K - want)) / n
    print("end to end (n %d, d %d): largest |lambda - lambda*| %.3g, ||K - K*||_F / n %.3g" % (n, d, err, bound))
    assert err <= bound, (n, d, err, bound)
    m = spectrum_metrics(K, n, d)
    assert m["feature_rank"] == min(5, d) and m["srank"] == min(5, d), (n, d, m["feature_rank"], m["srank"])


# =============================================================================== 3: the capture
def feature_dim(lib, cfg, which):
    d = C.c_int32(0)
    L.check(lib, lib.rb_learner_feature_dim(C.byref(cfg), which, C.byref(d)))
    return int(d.value)


def features(rig, states_buf, which, out_buf, ld):
    return rig.lib.rb_learner_features(rig.h, rig.mem.ptr(states_buf), which, rig.mem.ptr(out_buf), ld, rig.mem.stream)


def capture_check(lib, Mem, row):
    """Both layers, at ld = d + 4 and at ld = d: the B rows are bit-equal to rb_learner_debug_read (5; 6 + nconv - 1) after the same
    forward, the columns [d, ld) and what lies behind the last row keep their poison, no caller buffer changes, bad arguments are
    refused by name."""
    rig = RS.Rig(lib, Mem, row)
    m, B = rig.mem, rig.c["batch"]
    RS.load_net(rig, 5)
    before = rig.state()
    sbuf = m.upload(RS.random_states(rig.c, 17))
    nconv = len(rig.units) - 2
    dims = {HIDDEN: 2 * rig.c["hidden"], CONV: None}
    poison = np.float32(np.nan).view(np.uint32) | np.uint32(0x1234)
    for which in (HIDDEN, CONV):
        d = feature_dim(lib, rig.cfg, which)
        for ld in (d + 4, d):
            out = m.upload(np.full(B * ld + 8, poison, np.uint32).view(F32))
            L.check(lib, features(rig, sbuf, which, out, ld))
            m.sync()
            got = m.download(out)
            conv_acts, h = rig.activations()
            want = h if which == HIDDEN else conv_acts[nconv - 1].reshape(B, -1)
            assert want.shape == (B, d) and (dims[which] is None or dims[which] == d), (row, which, want.shape, d)
            rows = got[:B * ld].reshape(B, ld)
            assert np.array_equal(_u32(rows[:, :d]), _u32(want)), (row, which, ld, "the captured rows must equal debug_read bit for bit")
            assert np.all(_u32(rows[:, d:]) == poison) and np.all(_u32(got[B * ld:]) == poison), (row, which, ld, "pad columns were written")
            assert float(np.abs(want).sum()) > 0
    if row == "canon48":
        assert feature_dim(lib, rig.cfg, CONV) == 3136                   # 64 channels in runs of 49
    if row == "de48":
        assert feature_dim(lib, rig.cfg, HIDDEN) == 96
    RS.same(rig.state(), before, (row, "rb_learner_features must not write a caller's buffer"))
    d = feature_dim(lib, rig.cfg, HIDDEN)
    out = m.upload(np.full(B * d, poison, np.uint32).view(F32))
    for i, word in ((1, b"states_dev"), (2, b"which"), (3, b"out_dev"), (4, b"ld")):
        a = [rig.h, m.ptr(sbuf), HIDDEN, m.ptr(out), d, m.stream]
        a[i] = {1: None, 2: 2, 3: None, 4: d - 1}[i]
        assert lib.rb_learner_features(*a) == RB_ERR_INVALID and word in lib.rb_last_error(), word
    assert lib.rb_learner_feature_dim(C.byref(rig.cfg), 2, C.byref(C.c_int32(0))) == RB_ERR_INVALID
    assert lib.rb_learner_feature_dim(C.byref(rig.cfg), 0, None) == RB_ERR_INVALID
    m.sync()
    assert np.all(_u32(m.download(out)) == poison), "a refused call must write nothing"
    rig.close()


def _measure(lib, mem, ad, sbuf, bufs):
    """Everything this feature launches: both captures, the Gram matrix, the norms of parameters against target and of the gradient."""
    for which in (HIDDEN, CONV):
        L.check(lib, lib.rb_learner_features(ad.h, mem.ptr(sbuf), which, mem.ptr(bufs["phi"][which]), bufs["ld"][which], mem.stream))
    B = bufs["B"]
    L.check(lib, lib.rb_gram_f64(mem.ptr(bufs["phi"][HIDDEN]), B, bufs["d"][HIDDEN], bufs["ld"][HIDDEN], mem.ptr(bufs["K"]), mem.stream))
    L.check(lib, lib.rb_learner_tensor_norms(ad.h, mem.ptr(ad.p_on), mem.ptr(ad.p_tg), mem.ptr(bufs["norms"][0]), mem.stream))
    L.check(lib, lib.rb_learner_tensor_norms(ad.h, mem.ptr(ad.grads), None, mem.ptr(bufs["norms"][1]), mem.stream))
    mem.sync()


def _measure_bufs(lib, mem, ad):
    B = ad.c["batch"]
    d = {w: feature_dim(lib, ad.cfg, w) for w in (HIDDEN, CONV)}
    ld = {w: (d[w] + 3) // 4 * 4 + 4 for w in d}
    return dict(B=B, d=d, ld=ld, phi={w: mem.empty((B, ld[w]), np.float32) for w in d}, K=mem.empty((B, B), np.float64),
                norms=[mem.empty((len(ad.layout), 3), np.float64) for _ in range(2)])


def no_side_effects_check(lib, mem):
    """redo_scenarios.no_side_effects_check with this feature's launches in place of the activity and the mask: around the measurement
    parameters, target, moments, gradients, both noise buffers, the noise epoch, the step counter, the norm and the sink's tree are
    bit-identical; measured with a pass pending, the run goes on as its twin's."""
    c = DS.case_config("z51-a6")
    hs = [DS.ts_build(lib, mem, c, "_rank_se%d" % i, flags=L.LEARNER_DEFER_UPDATE) for i in range(2)]
    try:
        def rng(ad):
            s, e = C.c_uint64(0), C.c_uint64(0)
            L.check(lib, lib.rb_learner_get_rng(ad.h, C.byref(s), C.byref(e), mem.stream))
            return s.value, e.value
        for rp, ad, o, job in hs:
            DS.ts_call(lib, mem, c, rp, ad, o, job)
        rp, ad, o, job = hs[0]
        L.check(lib, lib.rb_learner_flush(ad.h, mem.stream))
        before, rng_before = DS.ts_state(mem, rp, ad, o), rng(ad)
        sbuf = mem.upload(RS.random_states(c, 99))
        bufs = _measure_bufs(lib, mem, ad)
        _measure(lib, mem, ad, sbuf, bufs)
        after, rng_after = DS.ts_state(mem, rp, ad, o), rng(ad)
        assert rng_before == rng_after
        for k in before:
            assert DS.same_bits(before[k], after[k]), "the rank / norm measurement changed %s" % k
        K, norms = mem.download(bufs["K"]), [mem.download(b) for b in bufs["norms"]]
        assert np.isfinite(K).all() and float(np.trace(K)) > 0 and all(np.isfinite(x).all() for x in norms)
        assert float(norms[0][:, 1].sum()) > 0 and float(norms[1][:, 0].sum()) > 0 and np.all(norms[1][:, 1] == 0)
        for rp, ad, o, job in hs:                                       # a pending pass runs first: twin 0 measures, twin 1 never does
            DS.ts_call(lib, mem, c, rp, ad, o, job)
        _measure(lib, mem, hs[0][1], sbuf, bufs)
        for rp, ad, o, job in hs:
            DS.ts_call(lib, mem, c, rp, ad, o, job)
        for rp, ad, o, job in hs:
            L.check(lib, lib.rb_learner_flush(ad.h, mem.stream))
        a, b = DS.ts_state(mem, *hs[0][:3]), DS.ts_state(mem, *hs[1][:3])
        for k in a:
            assert DS.same_bits(a[k], b[k]), "the steps after the measurement differ from the twin's in %s" % k
        assert rng(hs[0][1]) == rng(hs[1][1])
    finally:
        for i, (rp, ad, o, job) in enumerate(hs):
            ad.close(); rp.close()
            DS.drop_config("_rank_se%d" % i)


def refusal_check(lib, mem):
    """redo_scenarios.refusal_check for rb_learner_features: RB_ERR_STATE with the message of rb_learner_unit_activity while the
    gradients wait for rb_learner_finish_grads, nothing written, and the call works again afterwards."""
    import exchange_scenarios as XS
    c = DS.case_config("z51-a6")
    _cfg, online, target, steps = DS.learn_inputs(c, 11, steps=1)
    ad, name = DS.make_learner(lib, mem, "rank-xch", c)
    try:
        ad.load(online, target)
        stride = XS.exchange_layout(lib, ad)[0]
        lo, al = mem.upload(np.zeros(stride, dtype=np.float32)), mem.empty((2 * stride,), np.float32)
        L.check(lib, lib.rb_learner_set_exchange(ad.h, 2, mem.ptr(lo), mem.ptr(al)))
        st = steps[0]
        ad.reset_noise_online(st["raw_on"])
        ad.learn_only(st["batch"], st["raw_tg"])
        sbuf = mem.upload(RS.random_states(c, 5))
        d = feature_dim(lib, ad.cfg, HIDDEN)
        out = mem.upload(np.full((c["batch"], d), 7.0, F32))
        args = (ad.h, mem.ptr(sbuf), HIDDEN, mem.ptr(out), d, mem.stream)
        assert lib.rb_learner_features(*args) == RB_ERR_STATE
        msg = lib.rb_last_error()
        assert lib.rb_learner_unit_activity(ad.h, mem.ptr(sbuf), 0, mem.ptr(mem.empty((512,), np.float64)), mem.stream) == RB_ERR_STATE
        assert msg.replace(b"rb_learner_features", b"rb_learner_unit_activity") == lib.rb_last_error() and b"rb_learner_finish_grads" in msg
        mem.sync()
        assert np.all(mem.download(out) == 7.0)
        XS.fill(al, np.concatenate([mem.download(lo), mem.download(lo)]))
        L.check(lib, lib.rb_learner_finish_grads(ad.h, mem.stream))
        L.check(lib, lib.rb_learner_features(*args))
        mem.sync()
        assert np.isfinite(mem.download(out)).all()
    finally:
        lib.rb_learner_set_exchange(ad.h, 1, None, None)
        ad.close()
        DS.drop_config(name)


# =============================================================================== 4: per-tensor norms
def tensors_of(layout):
    """[(name, offset, count)] in rb_learner_param_layout's order."""
    return [(k, off, int(np.prod(shape))) for k, (off, shape) in layout.items()]


def scaled_buffers(rig, seed):
    """Two flat buffers with per-tensor scales 1e-8 .. 1e2 (optimizer_scenarios.make_grad); the alignment padding holds NaN."""
    a, b = S.make_grad(rig.layout, rig.n, seed, "scales"), S.make_grad(rig.layout, rig.n, seed + 1, "scales")
    covered = np.zeros(rig.n, bool)
    for _k, off, cnt in tensors_of(rig.layout):
        covered[off:off + cnt] = True
    assert not covered.all()
    a[~covered] = np.nan
    b[~covered] = np.nan
    return a, b


def norms_reference(layout, a, b):
    out = np.zeros((len(layout), 3), F64)
    for t, (_k, off, cnt) in enumerate(tensors_of(layout)):
        x = a[off:off + cnt].astype(F64)
        out[t, 0] = math.fsum(x * x)
        if b is not None:
            e = a[off:off + cnt].astype(np.longdouble) - b[off:off + cnt].astype(np.longdouble)
            out[t, 1] = float(np.sum(e * e, dtype=np.longdouble))
        out[t, 2] = float(np.abs(x).max())
    return out


def run_norms(rig, a, b):
    m = rig.mem
    ab, bb = m.upload(a), m.upload(b) if b is not None else None
    out = m.upload(np.full((len(rig.layout), 3), np.nan, F64))
    L.check(rig.lib, rig.lib.rb_learner_tensor_norms(rig.h, m.ptr(ab), m.ptr(bb) if bb is not None else None, m.ptr(out), m.stream))
    m.sync()
    return m.download(out)


def assert_norms(what, got, want, layout):
    counts = np.array([cnt for _k, _o, cnt in tensors_of(layout)], F64)
    worst = 0.0
    for col in (0, 1):
        err, bound = np.abs(got[:, col] - want[:, col]), (counts + 2) * U53 * want[:, col]
        pos = bound > 0
        worst = max(worst, float((err[pos] / bound[pos]).max()) if pos.any() else 0.0)
        assert np.all(err <= bound), (what, col, int(np.argmax(err - bound)))
    print("tensor norms %s: largest error / bound %.3g over %d tensors" % (what, worst, len(counts)))
    assert np.array_equal(_u64(got[:, 2]), _u64(want[:, 2])), (what, "max |a| must be exact")


def norms_check(lib, Mem, row):
    """With and without b against the reference; a repeat is bit-identical; a NaN planted in a (one tensor) and in b (another) makes
    exactly those tensors' rows NaN and leaves every other row's bits alone; the net has a tensor whose length is no multiple of 4
    and one that starts inside a quad; bad arguments are refused by name."""
    rig = RS.Rig(lib, Mem, row)
    m = rig.mem
    ts = tensors_of(rig.layout)
    assert any(cnt % 4 for _k, _o, cnt in ts) and any(off % 4 for _k, off, _c in ts), row
    assert any(cnt > 4096 for _k, _o, cnt in ts), "no tensor crosses a chunk"
    a, b = scaled_buffers(rig, 70)
    got = run_norms(rig, a, b)
    assert_norms(row, got, norms_reference(rig.layout, a, b), rig.layout)
    assert np.array_equal(_u64(run_norms(rig, a, b)), _u64(got)), "a repeated run must be bit-identical"
    alone = run_norms(rig, a, None)
    assert np.array_equal(_u64(alone[:, (0, 2)]), _u64(got[:, (0, 2)])) and np.all(alone[:, 1] == 0.0)
    same = run_norms(rig, a, a)
    assert np.all(same[:, 1] == 0.0)
    ka, kb = 1, len(ts) - 3
    a2, b2 = a.copy(), b.copy()
    a2[ts[ka][1] + ts[ka][2] - 1] = np.nan                              # the last element of one tensor
    b2[ts[kb][1]] = np.nan                                              # the first element of another, in b
    bad = run_norms(rig, a2, b2)
    hit = np.zeros(len(ts), bool)
    hit[[ka, kb]] = True
    assert np.isnan(bad[hit]).all() and np.array_equal(_u64(bad[~hit]), _u64(got[~hit])), (row, "a NaN must reach its own tensor only")
    ab, ob = m.upload(a), m.upload(np.full((len(ts), 3), 5.0, F64))
    for i, word in ((1, b"a_dev"), (3, b"out_dev")):
        args = [rig.h, m.ptr(ab), None, m.ptr(ob), m.stream]
        args[i] = None
        assert lib.rb_learner_tensor_norms(*args) == RB_ERR_INVALID and word in lib.rb_last_error(), word
    assert lib.rb_learner_tensor_norms(rig.h, m.ptr(ab) + 4, None, m.ptr(ob), m.stream) == RB_ERR_INVALID and b"a_dev" in lib.rb_last_error()
    assert lib.rb_learner_tensor_norms(rig.h, m.ptr(ab), m.ptr(ab) + 8, m.ptr(ob), m.stream) == RB_ERR_INVALID and b"b_dev" in lib.rb_last_error()
    m.sync()
    assert np.all(m.download(ob) == 5.0)
    rig.close()


def grad_norm_check(lib, mem, row):
    """One learn step, no clip (max_norm 1e30): sqrt(sum_t grad_sumsq) against the norm the learner reports, within the any-order
    float32 bound n_params 2^-24 relative."""
    c = RS.row_config(row)
    _cfg, online, target, steps = DS.learn_inputs(c, 23, steps=1)
    ad, name = DS.make_learner(lib, mem, "rank-gn-" + row, c)
    try:
        ad.load(online, target)
        st = steps[0]
        ad.reset_noise_online(st["raw_on"])
        ad.learn_only(st["batch"], st["raw_tg"])
        out = mem.upload(np.full((len(ad.layout), 3), np.nan, F64))
        L.check(lib, lib.rb_learner_tensor_norms(ad.h, mem.ptr(ad.grads), None, mem.ptr(out), mem.stream))
        norm = mem.empty((1,), np.float32)
        L.check(lib, lib.rb_learner_clip_grad(ad.h, 1e30, mem.ptr(norm), mem.stream))
        mem.sync()
        sums = mem.download(out)[:, 0]
        g = mem.download(ad.grads)
        assert_norms(row + " gradient", mem.download(out), norms_reference(ad.layout, g, None), ad.layout)
        mine, theirs = math.sqrt(float(sums.sum())), float(mem.download(norm)[0])
        bound = ad.n_params * 2.0 ** -24
        print("grad norm %s: sqrt(sum of tensor sums) %.9g, the learner's %.9g, relative difference / bound %.3g"
              % (row, mine, theirs, abs(mine - theirs) / theirs / bound))
        assert theirs > 0 and abs(mine - theirs) <= bound * theirs, (row, mine, theirs)
    finally:
        ad.close()
        DS.drop_config(name)
