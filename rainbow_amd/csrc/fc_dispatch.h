// fc_dispatch.h — the noisy-linear launches of the learner, forward and backward: take the plan (learner_plan.h), fill the argument
// structs, switch on the kernel id.  Included by learner.hip only, after conv_dispatch.h (plan_in), grad_finish.h (the kernels of
// the small passes) and noisy_rows.h (the per-row-noise kernels of fc_rows_fwd).
#pragma once
#include "learner_plan.h"

static NlWeights nl_h(const NetPtrs& p) {
  NlWeights w;
  w.mu = p.h_mu; w.sigma = p.h_sigma; w.eout = p.h_eout; w.ein = p.h_ein; w.bmu = p.h_bmu; w.bsigma = p.h_bsigma;
  return w;
}
static NlWeights nl_z(const NetPtrs& p) {
  NlWeights w;
  w.mu = p.z_mu; w.sigma = p.z_sigma; w.eout = p.z_eout; w.ein = p.z_ein; w.bmu = p.z_bmu; w.bsigma = p.z_bsigma;
  return w;
}

// Hidden and output layer of n_on online images + n_tg target images: features (act[nconv - 1] / feat_b) to the logits.
static int fc_forward(rb_learner* l, int n_on, int n_tg, const NetPtrs& on, const NetPtrs& tg, hipStream_t stream) {
  const Layout& L = l->L;
  const int NI = n_on + n_tg;
  const float* feat = l->act[L.nconv - 1];
  const FcFwdPlan p = plan_fc_fwd(plan_in(l), n_on, n_tg);
  if (p.h_kernel == FC_FWD_KGEMM) {
    {
      FcHFwdProb q;
      q.F = L.F; q.H = L.H; q.NI = NI; q.splits = l->caps.hs;
      q.n_img[0] = n_on; q.n_img[1] = n_tg; q.img_base[0] = 0; q.img_base[1] = n_on;
      q.feat = feat; q.net[0] = on; q.net[1] = tg; q.part = l->hpart;
      RB_LAUNCH((k_gemm<2, 2, FcHFwdProb>), p.hgrid, dim3(p.hblock), stream, q);
      RB_LAUNCH_CHECK();
      const int64_t total = (int64_t)NI * 2 * L.H;
      RB_LAUNCH(k_fc_h_finish, dim3((unsigned)rb_div_up(total, 256)), dim3(256), stream, (const float*)l->hpart, l->caps.hs, NI,
                2 * L.H, n_on, on, tg, l->h, (float*)nullptr);
      RB_LAUNCH_CHECK();
    }
    {
      FcZFwdProb q;
      q.H = L.H; q.Z = L.Z; q.NZ = L.NZ;
      q.n_img[0] = n_on; q.n_img[1] = n_tg; q.img_base[0] = 0; q.img_base[1] = n_on;
      q.h = l->h; q.net[0] = on; q.net[1] = tg; q.logits = l->logits;
      RB_LAUNCH((k_gemm<1, 1, FcZFwdProb>), p.zgrid, dim3(p.zblock), stream, q);
      RB_LAUNCH_CHECK();
    }
    return RB_OK;
  }
  if (p.block_copy) {
    RB_LAUNCH(k_block_copy, dim3((unsigned)rb_div_up((int64_t)NI * L.F, 256)), dim3(256), stream, feat, NI, L.F, l->feat_b);
    RB_LAUNCH_CHECK();
  }
  // hidden layer: both streams, both nets, weights streamed once, bias + ReLU fused, no partials (nl_fwd.h)
  NlFwdArgs a;
  a.x = l->feat_b;
  a.m_base[0] = 0; a.m_cnt[0] = n_on; a.m_base[1] = n_on; a.m_cnt[1] = n_tg;
  a.w[0] = nl_h(on); a.w[1] = nl_h(tg);
  a.K = L.F; a.n_groups = 2;
  const int ht16 = (int)rb_div_up(L.H, 16);
  a.grp[0] = NlRowGroup{0, L.H, 0, 0, 0};
  a.grp[1] = NlRowGroup{L.H, L.H, 0, L.F, ht16};
  a.out = l->h; a.out_blocked = l->h_b; a.ld_out = 2 * L.H; a.rows_total = NI; a.relu = 1;
  switch (p.h_kernel) {
    case FC_FWD_TILED: {
      FcGemmFwdArgs ga;
      ga.f = a;
      ga.mt[0] = p.mt[0]; ga.mt[1] = p.mt[1]; ga.nt = p.nt;
      ga.S = p.S; ga.part = l->gemm_part; ga.ctr = l->gemm_ctr;
      RB_LAUNCH_T("fc_h_fwd:k_fc_gemm_fwd", k_fc_gemm_fwd, p.hgrid, dim3(p.hblock), stream, ga);
      break;
    }
    case FC_FWD_NL3_4: RB_LAUNCH_T("fc_h_fwd:k_nl_fwd3", k_nl_fwd3<4>, p.hgrid, dim3(p.hblock), stream, a); break;
    default: RB_LAUNCH_T("fc_h_fwd:k_nl_fwd3", k_nl_fwd3<2>, p.hgrid, dim3(p.hblock), stream, a); break;
  }
  RB_LAUNCH_CHECK();
  // output layer: value rows read h[:, :H], advantage rows read h[:, H:]; bias fused
  NlFwdArgs z;
  z.x = l->h_b;
  z.m_base[0] = 0; z.m_cnt[0] = n_on; z.m_base[1] = n_on; z.m_cnt[1] = n_tg;
  z.w[0] = nl_z(on); z.w[1] = nl_z(tg);
  z.K = L.H; z.n_groups = 2;
  const int vt16 = (int)rb_div_up(L.Z, 16);
  z.grp[0] = NlRowGroup{0, L.Z, 0, 0, 0};
  z.grp[1] = NlRowGroup{L.Z, L.NZ - L.Z, L.H, L.H, vt16};
  z.out = l->logits; z.out_blocked = nullptr; z.ld_out = L.NZ; z.rows_total = NI; z.relu = 0;
  if (p.z_kernel == FC_FWD_NL3_4) { RB_LAUNCH_T("fc_z_fwd:k_nl_fwd3", k_nl_fwd3<4>, p.zgrid, dim3(p.zblock), stream, z); }
  else { RB_LAUNCH_T("fc_z_fwd:k_nl_fwd3", k_nl_fwd3<2>, p.zgrid, dim3(p.zblock), stream, z); }
  RB_LAUNCH_CHECK();
  return RB_OK;
}

// Forward of n_on online images + n_tg target images up to the logits.
static int forward(rb_learner* l, int n_on, int n_tg, const ImgSrc& src, const NetPtrs& on, const NetPtrs& tg,
                   hipStream_t stream) {
  for (int layer = 0; layer < l->L.nconv; ++layer) {
    int rc = conv_fwd(l, layer, n_on, n_tg, src, on, tg, stream);
    if (rc != RB_OK) return rc;
  }
  return fc_forward(l, n_on, n_tg, on, tg, stream);
}

// Arguments of one per-row-noise layer (noisy_rows.h) over n rows, which = 0: fc_z_v | fc_z_a, 1: fc_h_v | fc_h_a — for the streamed
// kernel (k-blocked operands, the hidden layer's epilogue writes the output layer's) and for the one-wave-per-cell fallback.
static NlRowsArgs nl_rows_args(rb_learner* l, const NetPtrs& on, int which, int n, const float* noise_rows) {
  const Layout& L = l->L;
  const NlWeights w = which ? nl_h(on) : nl_z(on);
  const int rows0 = which ? L.H : L.Z;             // weight rows of the value stream; the advantage stream's follow
  NlRowsArgs a;
  a.x = which ? l->feat_b : l->h_b; a.xs = which ? l->feat_s : l->h_s;
  a.mu = w.mu; a.sigma = w.sigma; a.bmu = w.bmu; a.bsigma = w.bsigma;
  a.noise_rows = noise_rows; a.n_noise = (int)L.n_noise; a.eout_off = (int)(which ? L.h_eout : L.z_eout);
  a.M = n; a.K = which ? L.F : L.H; a.n_groups = 2;
  a.grp[0] = NlRowGroup{0, rows0, 0, 0, 0};
  a.grp[1] = NlRowGroup{rows0, which ? L.H : L.NZ - L.Z, which ? 0 : L.H, a.K, (int)rb_div_up(rows0, 16)};
  a.out = which ? l->h : l->logits; a.out_blocked = which ? l->h_b : nullptr; a.out_scaled = which ? l->h_s : nullptr;
  a.next_ein_off = which ? (int)L.z_ein : 0; a.ld_out = which ? 2 * L.H : L.NZ; a.relu = which;
  return a;
}
static NlRowsGenericArgs nl_rows_generic_args(rb_learner* l, const NetPtrs& on, int which, int n, const float* noise_rows) {
  const Layout& L = l->L;
  const NlWeights w = which ? nl_h(on) : nl_z(on);
  NlRowsGenericArgs a;
  a.x = which ? l->act[L.nconv - 1] : l->h; a.ldx = which ? L.F : 2 * L.H;
  a.mu = w.mu; a.sigma = w.sigma; a.bmu = w.bmu; a.bsigma = w.bsigma;
  a.noise_rows = noise_rows; a.n_noise = (int)L.n_noise;
  a.ein_off = (int)(which ? L.h_ein : L.z_ein); a.eout_off = (int)(which ? L.h_eout : L.z_eout);
  a.M = n; a.N = which ? 2 * L.H : L.NZ; a.K = which ? L.F : L.H;
  a.split_row = which ? L.H : L.Z; a.x_off1 = which ? 0 : L.H; a.ein_off1 = a.K;
  a.out = which ? l->h : l->logits; a.ld_out = a.N; a.relu = which;
  return a;
}

// Hidden and output layer of n online images with row i under noise row i (rb_learner_act_batch_rows): features to the logits.
static int fc_rows_fwd(rb_learner* l, const ActRowsPlan& p, int n, const float* noise_rows, const NetPtrs& on, hipStream_t stream) {
  const Layout& L = l->L;
  if (p.kernel == ACT_ROWS_GENERIC) {
    const NlRowsGenericArgs h = nl_rows_generic_args(l, on, 1, n, noise_rows), z = nl_rows_generic_args(l, on, 0, n, noise_rows);
    RB_LAUNCH_T("fc_h_rows:k_nlr_generic", k_nlr_generic, p.hgrid, dim3(p.block), stream, h);
    RB_LAUNCH_CHECK();
    RB_LAUNCH_T("fc_z_rows:k_nlr_generic", k_nlr_generic, p.zgrid, dim3(p.block), stream, z);
    RB_LAUNCH_CHECK();
    return RB_OK;
  }
  RB_LAUNCH(k_block_copy_rows, p.copy_grid, dim3(256), stream, (const float*)l->act[L.nconv - 1], n, L.F, noise_rows, (int)L.n_noise,
            (int)L.h_ein, l->feat_b, l->feat_s);
  RB_LAUNCH_CHECK();
  const NlRowsArgs h = nl_rows_args(l, on, 1, n, noise_rows), z = nl_rows_args(l, on, 0, n, noise_rows);
  switch (p.kernel) {
    case ACT_ROWS_NLR_1:
      RB_LAUNCH_T("fc_h_rows:k_nlr_fwd", k_nlr_fwd<1>, p.hgrid, dim3(p.block), stream, h);
      RB_LAUNCH_CHECK();
      RB_LAUNCH_T("fc_z_rows:k_nlr_fwd", k_nlr_fwd<1>, p.zgrid, dim3(p.block), stream, z);
      break;
    default:
      RB_LAUNCH_T("fc_h_rows:k_nlr_fwd", k_nlr_fwd<2>, p.hgrid, dim3(p.block), stream, h);
      RB_LAUNCH_CHECK();
      RB_LAUNCH_T("fc_z_rows:k_nlr_fwd", k_nlr_fwd<2>, p.zgrid, dim3(p.block), stream, z);
      break;
  }
  RB_LAUNCH_CHECK();
  return RB_OK;
}

// Arguments of the weight-gradient problem of one noisy layer pair (which = 0: fc_z_v | fc_z_a, 1: fc_h_v | fc_h_a) over M
// reduction rows of dy / x, with its tiles (learner_plan.h plan_fc_dw_tiles).
struct FcDwPlan {
  NlDwArgs a;
  int dw_x, dw_y, slots;
};
static FcDwPlan fc_dw_plan(rb_learner* l, const NetPtrs& on, int which, const float* dy, const float* x, int M, int ct) {
  const Layout& L = l->L;
  FcDwPlan p;
  NlDwArgs& w = p.a;
  memset(&w, 0, sizeof(w));
  w.dy = dy; w.x = x; w.M = M; w.n_prob = 2; w.ct = ct; w.rpb = 0; w.bstride = 0; w.scale = 1.0f; w.sq_part = nullptr;
  w.noise_blocks = nullptr; w.eout_noff = 0; w.ein_noff = 0; w.norm_only = 0; w.no_sigma = 0;
  if (which == 0) {
    const int vt = (int)rb_div_up(L.Z, 16);
    w.ldy = L.NZ; w.ldx = 2 * L.H; w.K = L.H;
    w.prob[0] = NlDwProblem{0, L.Z, 0, 0, 0};
    w.prob[1] = NlDwProblem{L.Z, L.NZ - L.Z, L.H, L.H, vt};
    w.g_mu = l->grads + L.z_mu; w.g_sigma = l->grads + L.z_sigma; w.g_bmu = l->grads + L.z_bmu; w.g_bsigma = l->grads + L.z_bsigma;
    w.eout = on.z_eout; w.ein = on.z_ein;
  } else {
    const int ht = (int)rb_div_up(L.H, 16);
    w.ldy = 2 * L.H; w.ldx = L.F; w.K = L.F;
    w.prob[0] = NlDwProblem{0, L.H, 0, 0, 0};
    w.prob[1] = NlDwProblem{L.H, L.H, 0, L.F, ht};
    w.g_mu = l->grads + L.h_mu; w.g_sigma = l->grads + L.h_sigma; w.g_bmu = l->grads + L.h_bmu; w.g_bsigma = l->grads + L.h_bsigma;
    w.eout = on.h_eout; w.ein = on.h_ein;
  }
  const FcDwTiles t = plan_fc_dw_tiles(L, which, ct);
  p.dw_x = t.dw_x; p.dw_y = t.dw_y; p.slots = t.slots;
  return p;
}

// Backward of the two noisy layers (online net, images [0, B)): output layer, hidden layer, and — when its consumers do not form it
// themselves — d(conv output) into dact[nconv - 1].  Leaves the step's norm / deferral state in the handle.
// Streamed kernels: weight/bias grads and (ReLU-masked) input grads of a layer in ONE launch; the input-gradient chain
// (fc_z dX -> fc_h dX -> conv dX ...) is the critical path, the weight-gradient work rides in the same launches as block ranges
// (side streams measured slower, round 1).
static int fc_backward(rb_learner* l, const NetPtrs& on, float* loss_dev, hipStream_t stream) {
  const Layout& L = l->L;
  const int B = L.B;
  const float* feat = l->act[L.nconv - 1];
  l->exch_pending = 0;
  l->dw_deferred = 0;
  if (!l->caps.fast_fc) {
    const FcBwdPlan p = plan_fc_bwd(plan_in(l), false);
    l->lazy_dfeat = 0;
    l->norm_slots = 0;
    l->sink_done = 0;
    FcGradOut gz;
    gz.g_mu = l->grads + L.z_mu; gz.g_sigma = l->grads + L.z_sigma; gz.g_bmu = l->grads + L.z_bmu;
    gz.g_bsigma = l->grads + L.z_bsigma; gz.eout = on.z_eout; gz.ein = on.z_ein;
    {
      FcZDwProb q;
      q.B = B; q.H = L.H; q.Z = L.Z; q.NZ = L.NZ; q.dlogits = l->dlogits; q.h = l->h; q.o = gz;
      RB_LAUNCH((k_gemm<1, 2, FcZDwProb>), p.gz_dw, dim3(128), stream, q);
      RB_LAUNCH_CHECK();
    }
    {
      FcZDxProb q;
      q.B = B; q.H = L.H; q.Z = L.Z; q.NZ = L.NZ; q.dlogits = l->dlogits; q.h = l->h; q.net = on; q.dh = l->dh;
      RB_LAUNCH((k_gemm<1, 1, FcZDxProb>), p.gz_dx, dim3(64), stream, q);
      RB_LAUNCH_CHECK();
    }
    {
      FcHDwProb q;
      q.B = B; q.H = L.H; q.F = L.F; q.dh = l->dh; q.feat = feat;
      q.o.g_mu = l->grads + L.h_mu; q.o.g_sigma = l->grads + L.h_sigma; q.o.g_bmu = l->grads + L.h_bmu;
      q.o.g_bsigma = l->grads + L.h_bsigma; q.o.eout = on.h_eout; q.o.ein = on.h_ein;
      RB_LAUNCH((k_gemm<2, 2, FcHDwProb>), p.gh_dw, dim3(256), stream, q);
      RB_LAUNCH_CHECK();
    }
    {
      FcHDxProb q;
      q.B = B; q.H = L.H; q.F = L.F; q.splits = l->caps.xs; q.dh = l->dh; q.net = on; q.part = l->dfeat_part;
      RB_LAUNCH((k_gemm<1, 2, FcHDxProb>), p.gh_dx, dim3(128), stream, q);
      RB_LAUNCH_CHECK();
      const int64_t total = (int64_t)B * L.F;
      RB_LAUNCH(k_dfeat_finish, dim3((unsigned)rb_div_up(total, 256)), dim3(256), stream, (const float*)l->dfeat_part,
                l->caps.xs, total, feat, l->dact[L.nconv - 1]);
      RB_LAUNCH_CHECK();
    }
    return RB_OK;
  }
  // the write-back leaves this launch for the replay's stream (decided HERE, once: an expiry seen later only affects the next call)
  const PlanIn in = plan_in(l);
  const bool spec = l->spec_now && l->sink && B <= 256 && !in.exch && rb_replay_spec_allowed(l->sink);
  const FcBwdPlan p = plan_fc_bwd(in, spec);
  FcDwPlan zp = fc_dw_plan(l, on, 0, l->dlogits, l->h, B, p.z_ct);
  FcDwPlan hp = fc_dw_plan(l, on, 1, l->dh, feat, B, p.h_ct);
  NlDwArgs& zw = zp.a;
  NlDwArgs& hw_ = hp.a;
  hw_.norm_only = p.defer_dw ? 1 : 0;
  l->dw_deferred = p.defer_dw ? 1 : 0;
  hw_.no_sigma = p.implicit_sigma ? 1 : 0;
  l->sigma_implicit = p.implicit_sigma ? 1 : 0;
  zw.sq_part = p.fuse_norm ? l->norm_part : nullptr;
  hw_.sq_part = p.fuse_norm ? l->norm_part + p.z.slots : nullptr;
  l->norm_slots = p.norm_slots;
  l->norm_conv_base = p.norm_conv_base;
  // ---- output layer
  NlDxArgs zx;
  zx.dy = l->dlogits; zx.ldy = L.NZ; zx.M = B; zx.w = nl_z(on); zx.K = L.H; zx.n_prob = 2;
  zx.prob[0] = NlDxProblem{0, L.Z, 1 << 30, 0, 0, 0};
  zx.prob[1] = NlDxProblem{L.Z, L.NZ - L.Z, 1 << 30, L.H, L.H, L.H};
  zx.rows_per_split = (int)rb_div_up(L.NZ, 16) * 16;
  zx.out = l->dh; zx.ld_out = 2 * L.H; zx.mask_src = l->h;
  zx.dyT = l->dlogitsT; zx.ldyT = B; zx.outT = l->dhT;
  // ---- hidden layer
  NlDxArgs hx;
  hx.dy = l->dh; hx.ldy = 2 * L.H; hx.M = B; hx.w = nl_h(on); hx.K = L.F; hx.n_prob = 1;
  hx.prob[0] = NlDxProblem{0, 2 * L.H, L.H, 0, L.F, 0};
  hx.prob[1] = hx.prob[0];
  hx.rows_per_split = p.rows_per_split;
  hx.out = l->dfeat_part; hx.ld_out = L.F; hx.mask_src = nullptr;
  hx.dyT = l->dhT; hx.ldyT = B; hx.outT = nullptr;
  NlPriorityUpdate up;
  memset(&up, 0, sizeof(up));
  if (p.up_enabled) {
    up.enabled = 1; up.tree_idx = l->sink_idx; up.loss = loss_dev; up.n = B;
    if (rb_replay_internal_view(l->sink, &up.view, &up.omega) != RB_OK) {
      rb_set_error("rb_learner_learn: bad priority sink");
      return RB_ERR_STATE;
    }
  }
  NlPriorityUpdate none;
  memset(&none, 0, sizeof(none));
  if (spec) { none.go_flag = l->opt.spec_stall ? nullptr : l->go_flag; none.go_epoch = ++l->go_epoch; }
  if (p.z_kernel == FC_BWD_NL_TALL) { RB_LAUNCH_T("fc_z_bwd:k_nl_bwd", k_nl_bwd<true>, dim3(p.z_blocks), dim3(p.z_threads), stream, zw, zx, p.zg, none); }
  else { RB_LAUNCH_T("fc_z_bwd:k_nl_bwd", k_nl_bwd<false>, dim3(p.z_blocks), dim3(p.z_threads), stream, zw, zx, p.zg, none); }
  if (spec) {
    // the head is complete once the launch above has started: the write-back of THIS call and the draw of the NEXT one, on the
    // replay's stream, behind that launch's flag (submitted after it: a serialising profiler still terminates)
    RB_LAUNCH_CHECK();
    rb_spec_request q = l->spec_req;
    q.upd_idx = l->sink_idx; q.upd_loss = loss_dev; q.upd_n = B;
    q.go_flag = l->go_flag; q.go_epoch = l->go_epoch;
    const int rcs = rb_replay_spec_launch(l->sink, q);
    if (rcs != RB_OK) return rcs;
  }
  if (p.pack) {
    // every factor of the FC weight gradients exists now (dlogits, h, dh, feat rows [0, B)): pack them into this rank's
    // exchange block; the conv gradients join it at the end of the backward (k_reduce_conv_dw_all stores them twice)
    PackArgs pk;
    pk.src[0] = l->dlogits; pk.src[1] = l->h; pk.src[2] = l->dh; pk.src[3] = feat; pk.src[4] = l->n_online;
    pk.count[0] = (int64_t)B * L.NZ; pk.count[1] = (int64_t)B * 2 * L.H; pk.count[2] = (int64_t)B * 2 * L.H; pk.count[3] = (int64_t)B * L.F;
    pk.count[4] = L.n_noise;
    for (int i = 0; i < 5; ++i) pk.dst_off[i] = l->fact_off[i];
    pk.dst = l->fact_local;
    RB_LAUNCH(k_pack_factors, dim3(16, 5), dim3(256), stream, pk);
    RB_LAUNCH_CHECK();
    l->exch_pending = 1;
  }
  switch (p.h_kernel) {
    case FC_BWD_TILED: RB_LAUNCH_T("fc_h_bwd:k_fc_gemm_bwd", k_fc_gemm_bwd, dim3(p.h_blocks), dim3(p.h_threads), stream, hw_, hx, p.gg, up); break;
    case FC_BWD_NL: RB_LAUNCH_T("fc_h_bwd:k_nl_bwd", k_nl_bwd<false>, dim3(p.h_blocks), dim3(p.h_threads), stream, hw_, hx, p.hg, up); break;
    default: break;
  }
  l->sink_done = (up.enabled || spec) ? 1 : 0;
  RB_LAUNCH_CHECK();
  l->lazy_dfeat = p.lazy_dfeat ? 1 : 0;
  l->lazy_splits = p.hsplits;
  if (!l->lazy_dfeat) {
    const int64_t total = (int64_t)B * L.F;
    RB_LAUNCH(k_dfeat_finish, dim3((unsigned)rb_div_up(total, 256)), dim3(256), stream, (const float*)l->dfeat_part,
              p.hsplits, total, feat, l->dact[L.nconv - 1]);
    RB_LAUNCH_CHECK();
  }
  return RB_OK;
}
