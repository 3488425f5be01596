"""The C51 head (csrc/head.h k_head<ZI>, act_head.h rb_head_act_body) and the output layer in front of it over the accepted
(atoms, actions) range: one learn body and one act body, run on the host interpreter (test_head_shapes_emu.py) and on the
device (test_head_shapes_gpu.py) through the C ABI.  Every row of the table is the smallest shape on its side of a boundary.

Network of every row: data-efficient stack, history 4, multi_step 3, hidden 32 (fast_fc: the streamed output-layer kernels),
batch 5 (odd; the z_tall backward), support [-10, 10].  Variants: hidden 48 (H % 32 != 0: the generic k_gemm / k_nlr_generic
output layer) and batch 33 (B > 32: k_nl_bwd<false> with RB_NL_DX_M64_ST8, weight-gradient body not pipelined).

  case            Z    A   NZ   crosses                                                                    seed  min gap   ReLU margin
  z2-a1           2    1     4  minimum of both; one action (dueling mean = the advantage itself)             1  inf       4.655e-05
  z64-a7         64    7   512  last ballot-scatter Z (lane 63 run start, 64-atom run); 15 tasks, no wrap     1  1.022e-02 4.655e-05
  z65-a8         65    8   585  first ZI = 2, first serial scatter; 17 tasks on 16 waves                      1  1.185e-02 4.655e-05
  z128-a10      128   10  1408  ZI = 2 full; NZ = RB_HEAD_MAX_NZ; act launch: 352 units > 256 workgroups      1  3.679e-02 4.655e-05
  z129-a9       129    9  1290  first ZI = 4                                                                  3  6.660e-02 1.291e-04
  z256-a4       256    4  1280  ZI = 4 full; RB_MAX_ATOMS                                                     2  1.811e-02 3.244e-04
  z51-a18        51   18   969  full Atari action set: 37 tasks, three rounds                                 1  2.253e-02 4.655e-05
  z21-a64        21   64  1365  RB_MAX_ACTIONS: 129 tasks, s_ev full                                          8  2.532e-02 4.622e-04
  z65-a8-h48     65    8   585  hidden 48                                                                     3  1.026e-02 3.006e-04
  z128-a10-h48  128   10  1408  hidden 48                                                                     2  1.733e-02 3.911e-05
  z128-a10-b33  128   10  1408  batch 33                                                                      1  3.679e-02 2.406e-05

Conditioning (asserted by the bodies, "ill-conditioned seed"; no case is skipped, masked or retried): the seed of a shape
gives EVERY argmax — a* of every learn row, the action of every act call — a top-two gap of at least 1e-4 of the support's
width (2e-3) in the float64 reference, and the learn step a hidden_relu_margin above RELU_MARGIN.  The seeds were chosen on
the CPU (`PYTHONPATH=.:tests python tests/head_shapes_scenarios.py seeds`: first seed from 1 whose ORACLE figures meet both with a factor 2.5
to spare), then confirmed on the host interpreter's own logits; "min gap" above is the smallest gap over the learn rows and
the act calls of the case, as the host interpreter run printed it.

Tolerances.  m against head_oracle: rtol 1e-4, atol 1e-6 (test_learn_step_at_baseline_shapes_matches_oracle); loss: rtol 2e-5,
atol 1e-6; row sums of m and pns_a: 1 within 2e-6 (test_projection_known_answers); gradients: helpers.assert_learn_trace_matches'
rtol 2e-4, atol 5e-6 max|g|; act q: rtol 2e-5, atol 1e-6 (test_act_path_single_equals_batched; the per-row-noise path's own
RTOL / ATOL of noise_rows_scenarios.py are the same numbers).  log_ps_a and pns_a have no precedent against a float64 head:
  error measure   log_ps_a: |got - want| / max(1, |want|)      pns_a: |got - want| / want
  (log p is a difference of O(1) float32 values, its rounding scales with its own magnitude once that exceeds 1; p = exp(log p),
  so its RELATIVE error is log p's absolute one)
  measured, largest over all rows and atoms      log_ps_a     pns_a
    host interpreter, the whole table above      1.260e-07    1.781e-07     (z129-a9; z128-a10-h48)
    MI355X at (51, 6), seed 3 — the shape every  1.050e-07    1.547e-07
    other test runs: the baseline, not the code under test
  bound = 4 x the larger of the two              5.040e-07    7.124e-07     (margin for expf / logf differences between the builds)
  (for the record, not part of the bound: the MI355X over the whole table measured 1.450e-07 and 1.781e-07)"""

import numpy as np

import head_oracle as HO
import scenarios
from cabi_adapter import CAbiLearnAdapter
from eval_scenarios import varied_states
from oracle import learner_oracle as O
from rainbow_amd import _lib as L

BASE = dict(architecture="data-efficient", hidden=32, batch=5, multi_step=3, discount=0.99, history=4, v_min=-10.0, v_max=10.0)

# case id: (atoms, actions, overrides of BASE, seed)
CASES = {
    "z2-a1": (2, 1, {}, 1),
    "z64-a7": (64, 7, {}, 1),
    "z65-a8": (65, 8, {}, 1),
    "z128-a10": (128, 10, {}, 1),
    "z129-a9": (129, 9, {}, 3),
    "z256-a4": (256, 4, {}, 2),
    "z51-a18": (51, 18, {}, 1),
    "z21-a64": (21, 64, {}, 8),
    "z65-a8-h48": (65, 8, dict(hidden=48), 3),
    "z128-a10-h48": (128, 10, dict(hidden=48), 2),
    "z128-a10-b33": (128, 10, dict(batch=33), 1),
}
BASELINE_CASE = ("z51-a6", (51, 6, {}, 3))      # the shape every other test runs: measured, not part of the table

GAP_SHARE = 1e-4                 # of the support's width
LOGP_BOUND = 4 * 1.260e-07       # from the measurements in the header
PNS_BOUND = 4 * 1.781e-07
ACT_RTOL, ACT_ATOL = 2e-5, 1e-6
N_STATES = 3


def case_config(case):
    atoms, actions, over, seed = CASES[case] if case in CASES else dict([BASELINE_CASE])[case]
    return dict(BASE, atoms=atoms, actions=actions, **over), seed


def make_learner(lib, mem, case, c):
    name = "_head_" + case
    scenarios.LEARN_CONFIGS[name] = c
    try:
        return CAbiLearnAdapter(lib, mem, name)
    finally:
        del scenarios.LEARN_CONFIGS[name]


def relu_margin_floor():
    from test_learner_gpu import RELU_MARGIN
    return RELU_MARGIN


def learn_inputs(c, seed):
    """Seeded parameters, noise and the corner-case batch of scenarios.make_batch, with row 0 (terminal) moved onto an atom:
    make_batch's R = 0 is an integer b only for odd Z.  The first k from mid support whose float32 chain gives b == k exactly
    is taken (none for Z = 2: there the clamped rows are the integer-b rows)."""
    cfg = O.Config(**c)
    online, target = O.init_params(cfg, seed), O.init_params(cfg, seed + 1000)
    rs = np.random.RandomState(seed + 2000)
    draws = O.noise_draw_count(cfg)
    raw_on, raw_tg = rs.randn(draws).astype(np.float32), rs.randn(draws).astype(np.float32)
    batch = scenarios.make_batch(c, seed + 3000)
    Z = c["atoms"]
    dz = (c["v_max"] - c["v_min"]) / (Z - 1)
    for k in range((Z - 1) // 2, Z - 1):
        if k < 1:
            continue
        R = np.float32(c["v_min"] + k * dz)
        if float(HO.bins32(cfg, [R], [0.0])[1][0, 0]) == float(k):
            batch["returns"][0] = R
            break
    return cfg, online, target, raw_on, raw_tg, batch


def row_kinds(cfg, batch):
    """(terminal rows, rows with an integer b, rows clipped at Vmax) as boolean masks."""
    raw, b, _l, _u = HO.bins32(cfg, batch["returns"], batch["nonterminals"])
    terminal = np.asarray(batch["nonterminals"]).reshape(-1) == 0
    return terminal, (b == np.floor(b)).any(axis=1), (raw > np.float32(cfg.v_max)).any(axis=1)


def logp_error(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(1.0, np.abs(want))).max())


def pns_error(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(want, 1e-300)).max())


# =============================================================================== learn
def check_learn(lib, mem, case):
    """One learn step of the case; the head against head_oracle on the DEVICE's logits, loss / norm / every clipped gradient
    against the float32 oracle, the output layer's bias gradient against head_oracle's dlogits summed over the batch."""
    c, seed = case_config(case)
    cfg, online, target, raw_on, raw_tg, batch = learn_inputs(c, seed)
    B, Z, A = c["batch"], c["atoms"], c["actions"]
    NZ = Z * (A + 1)
    terminal, integer_b, clipped_hi = row_kinds(cfg, batch)
    assert terminal.any() and integer_b.any() and clipped_hi.any(), (terminal, integer_b, clipped_hi)
    ad = make_learner(lib, mem, case, c)
    try:
        ad.load(online, target)
        ad.reset_noise_online(raw_on)
        got = ad.learn_step(batch, raw_tg)
        logits = ad.debug(4, (3 * B, NZ), np.float32)
        a_star = ad.debug(2, (B,), np.int32)
        log_ps_a, pns_a, m = (ad.debug(k, (B, Z), np.float32) for k in (0, 3, 1))
    finally:
        ad.close()
    assert np.isfinite(logits).all()
    ref = HO.head(cfg, logits, batch["actions"], batch["returns"], batch["nonterminals"], batch["weights"])
    want = O.learn(cfg, online, target, O.make_noise(cfg, raw_on), O.make_noise(cfg, raw_tg), batch)
    width = c["v_max"] - c["v_min"]
    e_logp, e_pns = logp_error(log_ps_a, ref["log_ps_a"]), pns_error(pns_a, ref["pns_a"])
    print("head_shapes learn %s seed %d: min a* gap %.3e, relu margin %.3e, log_ps_a error %.3e, pns_a error %.3e"
          % (case, seed, ref["gap"].min(), want["hidden_relu_margin"], e_logp, e_pns))
    assert ref["gap"].min() >= GAP_SHARE * width, "ill-conditioned seed: a* top-two gap %.3e" % ref["gap"].min()
    assert want["hidden_relu_margin"] > relu_margin_floor(), \
        "ill-conditioned seed: a hidden pre-activation within rounding noise of 0 (%.3e)" % want["hidden_relu_margin"]
    # the bins are discrete: head_oracle's float32 chain and the oracle's agree exactly
    assert np.array_equal(ref["l"], want["l"]) and np.array_equal(ref["u"], want["u"])
    # ---- the head against the float64 head on the same logits
    assert np.array_equal(a_star.astype(np.int64), ref["a_star"]), (a_star.tolist(), ref["a_star"].tolist())
    assert e_logp <= LOGP_BOUND, "log_ps_a error %.3e > %.3e" % (e_logp, LOGP_BOUND)
    assert e_pns <= PNS_BOUND, "pns_a error %.3e > %.3e" % (e_pns, PNS_BOUND)
    np.testing.assert_allclose(m, ref["m"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(got["loss"], ref["loss"], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(m.sum(1), 1.0, rtol=0, atol=2e-6)
    np.testing.assert_allclose(pns_a.sum(1), 1.0, rtol=0, atol=2e-6)
    # ---- the whole step against the float32 oracle: loss, norm, every clipped gradient (dlogits, its [NZ][B] copy, the output
    # layer's dW / dX at this width)
    assert np.array_equal(a_star.astype(np.int64), want["a_star"])
    total, clipped = O.clip_grads(want["grads"], scenarios.LEARN_HYPER["norm_clip"])
    np.testing.assert_allclose(got["loss"], want["loss"], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(got["grad_norm"], total, rtol=2e-5)
    for k, g in clipped.items():
        np.testing.assert_allclose(got["grads"][k], g, rtol=2e-4, atol=5e-6 * float(np.abs(g).max()) + 1e-12, err_msg=k)
    # ---- dlogits itself, in float64: the output layer's bias gradient is its sum over the batch
    coef = min(1.0, scenarios.LEARN_HYPER["norm_clip"] / (float(got["grad_norm"]) + 1e-6))
    db = np.concatenate([got["grads"]["fc_z_v.bias_mu"], got["grads"]["fc_z_a.bias_mu"]]).astype(np.float64) / coef
    want_db = ref["dlogits"].sum(axis=0)
    np.testing.assert_allclose(db, want_db, rtol=2e-4, atol=5e-6 * float(np.abs(want_db).max()) + 1e-12)


# =============================================================================== act
_ACT_ORACLE = {}


def act_inputs(c, seed):
    cfg = O.Config(**c)
    params = O.init_params(cfg, seed)
    rs = np.random.RandomState(seed + 4000)
    draws = O.noise_draw_count(cfg)
    raw_shared = rs.randn(draws).astype(np.float32)
    raw_rows = rs.randn(N_STATES, draws).astype(np.float32)
    states = varied_states(N_STATES, c["history"], seed=seed + 5000)
    return cfg, params, raw_shared, raw_rows, states


def act_oracle(case, seed=None):
    """O.act per state under the shared noise, in eval mode and under the state's own noise row, with the top-two gap of the
    per-action values (float64 sum of the oracle's probabilities).  Once per case and process."""
    c, own = case_config(case)
    seed = own if seed is None else seed
    if (case, seed) not in _ACT_ORACLE:
        import torch
        cfg, params, raw_shared, raw_rows, states = act_inputs(c, seed)
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


def _same(got_a, got_q, want, what):
    got_a = np.asarray(got_a, dtype=np.int64).reshape(-1)
    assert (got_a >= 0).all(), "%s: action %s — an in-launch wait of the act path expired" % (what, got_a.tolist())
    assert np.array_equal(got_a, want["a"]), (what, got_a.tolist(), want["a"].tolist())
    np.testing.assert_allclose(np.asarray(got_q, dtype=np.float32).reshape(-1), want["q"], rtol=ACT_RTOL, atol=ACT_ATOL, err_msg=what)


def check_act(lib, mem, case, monkeypatch):
    """Three states, noisy and eval mode: rb_learner_act (as one launch, and with RB_OPTS act_fused=0 as one launch per phase of
    the same kernel; the two also against each other, bit for bit — on the host interpreter both run one launch per phase, so
    there that holds by construction), rb_learner_act_batch, rb_learner_act_batch_eps at epsilon 0, rb_learner_act_batch_rows —
    each (action, q) against O.act."""
    c, seed = case_config(case)
    cfg, params, raw_shared, raw_rows, states = act_inputs(c, seed)
    ora = act_oracle(case)
    width = c["v_max"] - c["v_min"]
    gap = min(float(ora[k]["gap"].min()) for k in ora)
    print("head_shapes act %s seed %d: min action gap %.3e" % (case, seed, gap))
    assert gap >= GAP_SHARE * width, "ill-conditioned seed: action top-two gap %.3e" % gap
    ad = make_learner(lib, mem, case, c)
    monkeypatch.setenv("RB_OPTS", "act_fused=0")
    unfused = make_learner(lib, mem, case, c)
    monkeypatch.delenv("RB_OPTS")
    m = mem
    try:
        for x in (ad, unfused):
            x.load(params, params)
            x.reset_noise_online(raw_shared)
        st = m.upload(states)
        for noisy in (1, 0):
            want = ora["noisy" if noisy else "eval"]
            got = []
            for x, what in ((ad, "rb_learner_act"), (unfused, "rb_learner_act act_fused=0")):
                single = [x.act(s, bool(noisy)) for s in states]
                got.append(([s[0] for s in single], np.asarray([s[1] for s in single], dtype=np.float32)))
                _same(got[-1][0], got[-1][1], want, "%s noisy=%d" % (what, noisy))
            # the two launch forms run the same bodies in the same order: equal actions, q equal as 32-bit words
            assert got[0][0] == got[1][0], ("noisy=%d" % noisy, got[0][0], got[1][0])
            assert np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32)), \
                ("noisy=%d: q of one launch / of one launch per phase" % noisy, [float(v).hex() for v in got[0][1]], [float(v).hex() for v in got[1][1]])
            a, q = ad.act_batch(states, bool(noisy))
            _same(a, q, want, "rb_learner_act_batch noisy=%d" % noisy)
            a, q, e = m.upload(np.full(N_STATES, -3, np.int32)), m.empty((N_STATES,), np.float32), m.empty((N_STATES,), np.uint8)
            L.check(lib, lib.rb_learner_act_batch_eps(ad.h, m.ptr(st), N_STATES, noisy, 0.0, 77, 3, 0, m.ptr(a), m.ptr(q), m.ptr(e), m.stream))
            m.sync()
            assert not m.download(e).any()
            _same(m.download(a), m.download(q), want, "rb_learner_act_batch_eps noisy=%d" % noisy)
        # one noise sample per row, filled from the injected normals as noise_rows_scenarios.RowsContext does
        raw = m.upload(raw_rows)
        rows = m.empty((N_STATES, ad.n_noise), np.float32)
        L.check(lib, lib.rb_learner_noise_rows(ad.h, N_STATES, 0, 0, 0, m.ptr(raw), m.ptr(rows), m.stream))
        a, q = m.upload(np.full(N_STATES, -3, np.int32)), m.empty((N_STATES,), np.float32)
        L.check(lib, lib.rb_learner_act_batch_rows(ad.h, m.ptr(st), N_STATES, m.ptr(rows), m.ptr(a), m.ptr(q), m.stream))
        m.sync()
        _same(m.download(a), m.download(q), ora["rows"], "rb_learner_act_batch_rows")
    finally:
        ad.close()
        unfused.close()


# =============================================================================== seed search (CPU, oracle only)
def oracle_figures(case, seed):
    """(min a* gap over the learn rows, relu margin, min action gap over the act calls) of `seed`, from the oracle alone."""
    import torch
    c, _ = case_config(case)
    cfg, online, target, raw_on, raw_tg, batch = learn_inputs(c, seed)
    want = O.learn(cfg, online, target, O.make_noise(cfg, raw_on), O.make_noise(cfg, raw_tg), batch)
    with torch.no_grad():
        p = {k: torch.as_tensor(np.ascontiguousarray(v)) for k, v in online.items()}
        ps = O.forward(cfg, p, O.make_noise(cfg, raw_on), torch.as_tensor(batch["next_states"]).to(torch.float32).div(255))
    ev = (ps.numpy().astype(np.float64) * HO.support32(cfg).astype(np.float64)).sum(axis=2)
    ora = act_oracle(case, seed)
    return float(HO.top2_gap(ev).min()), float(want["hidden_relu_margin"]), min(float(ora[k]["gap"].min()) for k in ora)


def find_seed(case, spare=2.5):
    width = BASE["v_max"] - BASE["v_min"]
    for seed in range(1, 400):
        gap, margin, act_gap = oracle_figures(case, seed)
        if min(gap, act_gap) >= spare * GAP_SHARE * width and margin > spare * relu_margin_floor():
            return seed, gap, margin, act_gap
    raise AssertionError("no seed below 400 for " + case)


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["seeds"]:
        for case in list(CASES) + [BASELINE_CASE[0]]:
            print(case, "seed %d: a* gap %.3e, relu margin %.3e, action gap %.3e" % find_seed(case))
