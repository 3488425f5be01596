// learner.hip — the Rainbow learn step on MI355X (gfx950): three forwards, double-Q select,
// C51 projection, importance-weighted cross-entropy and the full backward, as hand-written
// HIP over flat float32 parameter / gradient / noise buffers borrowed from the caller.
//
// Reference being replaced: model.py (NoisyLinear, DQN) and agent.py:61-98.  The reference
// issues ~1750 framework ops per learn(); here the step is a fixed chain of 14 launches after the sampler
// (DESIGN.md §3 has the table with what bounds each):
//   conv fwd x L (conv_fwd.h and its sections conv_fwd_*.h: operands in LDS, 8 waves split K or whole-K tiles)
//   -> fc_h, fc_z forward (nl_fwd.h k_nl_fwd3: weights streamed once, whole K per block, no partials)
//   -> head (dueling + softmaxes + double-Q + projection + loss + dlogits, one workgroup per sample, atom bins in LDS)
//   -> fc_z backward (dW || dX in one launch) -> fc_h backward (dW || dX || the sum-tree priority write-back)
//   -> dfeat finish -> conv dX x (L-1) -> every conv dW in one launch -> slice reduction
//   -> clip + Adam in one pass (norm from per-producer partials; optional fused fc_h weight gradient).
// All contractions run on v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32 (exact f32: parity with the float32 reference
// is the contract).  gemm_core.h + learner_problems.h remain the generic fallback for shapes the fast kernels refuse.
//
// This file keeps the handle's lifecycle and the step itself (learn_impl, train_step_impl and their entry points).  Its sections:
//   learner_internal.h  layout, RB_OPTS, the handle          learner_plan.h     which kernel a shape reaches (pure functions)
//   head.h / grad_finish.h / adam_kernels.h / noise_kernel.h  kernels           conv_dispatch.h / fc_dispatch.h   the launches
//   noisy_rows.h  the per-row-noise act layers (kernels)         learn_stats.h  the step records and the held-out loss
//   param_reset.h  shrink-and-perturb resets                     unit_recycle.h  dormant units: activity, mask, targeted reset
//   feature_gram.h  feature capture and the f64 Gram matrix      tensor_norms.h  per-tensor norms of a flat buffer
//   optimizer_host.h / act_host.h / exchange_host.h / layout_api.h / launch_plan_debug.h   the other entry points, by concern
// Each is included HERE and nowhere else (they define non-template kernels and static functions).
#include "learner_internal.h"
#include "kernel_stamp.h"
#include "learner_plan.h"
#include "noise_kernel.h"
#include "grad_finish.h"
#include "head.h"
#include "adam_kernels.h"
#include "noisy_rows.h"
#include "conv_dispatch.h"
#include "fc_dispatch.h"
#include "optimizer_host.h"
#include "param_reset.h"
#include "learn_stats.h"
#include "unit_recycle.h"
#include "feature_gram.h"
#include "tensor_norms.h"
#include "act_host.h"
#include "exchange_host.h"
#include "layout_api.h"
#include "launch_plan_debug.h"

#if defined(RB_STAMP)
__device__ long long g_span[64];
extern "C" int rb_debug_spans(long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_span), sizeof(long long) * 64) != hipSuccess) return -2;
  if (reset) {
    long long init[64];
    for (int i = 0; i < 64; ++i) init[i] = (i & 1) ? 0 : 0x7fffffffffffffffLL;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_span), init, sizeof(init)) != hipSuccess) return -2;
  }
  return 0;
}
__device__ long long g_cstamp[64];
extern "C" int rb_debug_cstamps(long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cstamp), sizeof(long long) * 64) == hipSuccess ? 0 : -2; }
__device__ long long g_wgt[RB_WGT_KERNELS][RB_WGT_WGS][8];
extern "C" int rb_debug_wgtrace(long long* out, int clear) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wgt), sizeof(long long) * RB_WGT_KERNELS * RB_WGT_WGS * 8) != hipSuccess) return -2;
  if (clear) { void* p = nullptr; if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_wgt)) != hipSuccess || hipMemset(p, 0, sizeof(long long) * RB_WGT_KERNELS * RB_WGT_WGS * 8) != hipSuccess) return -2; }
  return 0;
}
#endif
// torch.linspace(start, end, steps) float32 semantics (agent.py:18): step = (end-start)/(steps-1);
// first half counts up from start, second half counts down from end.
static void linspace_f32(float start, float end, int steps, float* out) {
  const float step = (end - start) / (float)(steps - 1);
  const int half = steps / 2;
  for (int i = 0; i < steps; ++i)
    out[i] = i < half ? start + step * (float)i : end - step * (float)(steps - i - 1);
}

extern "C" {

int rb_learner_destroy(rb_learner_t* l) {
  if (!l) return RB_OK;
  float** owned[] = {&l->feat_b, &l->h_b, &l->act[0], &l->act[1], &l->act[2], &l->dact[0], &l->dact[1], &l->dact[2], &l->hpart, &l->h,
                     &l->logits, &l->dlogits, &l->dlogitsT, &l->dh, &l->dhT, &l->dfeat_part, &l->dw_part[0], &l->dw_part[1], &l->dw_part[2],
                     &l->conv_wT[0], &l->conv_wT[1], &l->conv_wT[2],
                     &l->log_ps_a, &l->pns_a, &l->m, &l->support, &l->zero_noise, &l->norm_part, &l->gemm_part, &l->noise_snap, &l->feat_s, &l->h_s};
  for (float** p : owned)
    if (*p) rb_dev_free(*p);
  if (l->a_star) rb_dev_free(l->a_star);
  if (l->noise_ctr) rb_dev_free(l->noise_ctr);
  if (l->act_ctr) rb_dev_free(l->act_ctr);
  if (l->gemm_ctr) rb_dev_free(l->gemm_ctr);
  if (l->job_dev) rb_dev_free(l->job_dev);
  if (l->status_copy) rb_dev_free(l->status_copy);
  if (l->adam_args_dev) rb_dev_free(l->adam_args_dev);
  if (l->go_flag) rb_dev_free(l->go_flag);
  if (l->stats_rows) rb_dev_free(l->stats_rows);
  if (l->stats_ticket) rb_dev_free(l->stats_ticket);
  if (l->ones) rb_dev_free(l->ones);
  tensor_norms_release(l);
  delete l;
  return RB_OK;
}

static NoiseMap noise_map(const Layout& L) {
  NoiseMap map;
  const int64_t counts[8] = {L.F, L.H, L.F, L.H, L.H, L.Z, L.H, (int64_t)L.A * L.Z};
  const int64_t dst[8] = {L.h_ein, L.h_eout, L.h_ein + L.F, L.h_eout + L.H, L.z_ein, L.z_eout, L.z_ein + L.H, L.z_eout + L.Z};
  map.seg_begin[0] = 0;
  for (int i = 0; i < 8; ++i) { map.seg_begin[i + 1] = map.seg_begin[i] + (int32_t)counts[i]; map.dst[i] = (int32_t)dst[i]; }
  return map;
}

static NoiseJob make_noise_job(rb_learner* l, int which) {
  NoiseJob j;
  j.noise = which == 1 ? l->n_target : l->n_online;
  j.noise2 = which == 2 ? l->n_target : nullptr;
  j.map = noise_map(l->L);
  j.seed = l->seed; j.ctr = l->noise_ctr;
  j.nblk = (int)rb_div_up(j.map.seg_begin[8], 256); j.nets = which == 2 ? 2 : 1;
  j.dev = l->job_dev + which;
  j.adam_dev = nullptr; j.adam_blocks = 0; j.adam_ema = 0;
  return j;
}
// device copies of the three job variants (a hosting kernel reads them through NoiseJob::dev): at creation and whenever the
// seed changes — never from rb_learner_noise_job, which may be called while a stream is capturing
static int upload_noise_jobs(rb_learner* l) {
  if (!l->job_dev) RB_HIP_TRY(rb_dev_malloc((void**)&l->job_dev, 3 * sizeof(NoiseJob)));
  NoiseJob j[3];
  for (int which = 0; which < 3; ++which) j[which] = make_noise_job(l, which);
  RB_HIP_TRY(hipMemcpy(l->job_dev, j, sizeof(j), hipMemcpyHostToDevice));
  return RB_OK;
}

int rb_learner_noise_job(rb_learner_t* l, int32_t which, rb_noise_job_t* out) {
  RB_REQUIRE(l && out, "rb_learner_noise_job: NULL argument");
  RB_REQUIRE(which >= 0 && which <= 2, "rb_learner_noise_job: which must be 0 (online), 1 (target) or 2 (both)");
  static_assert(sizeof(NoiseJob) <= sizeof(rb_noise_job_t), "rb_noise_job_t too small");
  RB_REQUIRE(l->job_dev != nullptr, "rb_learner_noise_job: handle has no device job table");
  const NoiseJob j = make_noise_job(l, which);
  memset(out, 0, sizeof(*out));
  memcpy(out, &j, sizeof(j));
  return RB_OK;
}

int rb_learner_reset_noise(rb_learner_t* l, int32_t which, const float* raw_normals_dev, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_reset_noise: NULL handle");
  RB_REQUIRE(which >= 0 && which <= 2, "rb_learner_reset_noise: which must be 0 (online), 1 (target) or 2 (both)");
  RB_REQUIRE(!(which == 2 && raw_normals_dev), "rb_learner_reset_noise: injected normals need one call per net");
  const NoiseMap map = noise_map(l->L);
  float* noise = which == 1 ? l->n_target : l->n_online;
  float* noise2 = which == 2 ? l->n_target : nullptr;
  RB_LAUNCH(k_noise, dim3((unsigned)rb_div_up(map.seg_begin[8], 256), which == 2 ? 2u : 1u), dim3(256), stream, noise, noise2,
            raw_normals_dev, map, l->seed, l->noise_ctr);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

// One noise sample per ROW for rb_learner_act_batch_rows (include/rainbow_hip.h; noisy_rows.h k_noise_rows): keyed by (seed, round,
// row) alone — the learner's epoch counter is neither read nor advanced.
int rb_learner_noise_rows(rb_learner_t* l, int32_t rows, int32_t row0, uint64_t rng_seed, uint64_t rng_round,
                          const float* raw_normals_dev, float* noise_rows_dev, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_noise_rows: NULL handle (l)");
  RB_REQUIRE(noise_rows_dev != nullptr, "rb_learner_noise_rows: NULL noise_rows_dev");
  RB_REQUIRE(rows >= 1 && rows <= 256, "rb_learner_noise_rows: rows must be in [1, 256], got %d", (int)rows);
  RB_REQUIRE(row0 >= 0, "rb_learner_noise_rows: row0 must be >= 0, got %d", (int)row0);
  const NoiseMap map = noise_map(l->L);
  const int n_noise = (int)l->L.n_noise;
  RB_LAUNCH(k_noise_rows, dim3((unsigned)rb_div_up(n_noise, 256), (unsigned)rows), dim3(256), stream, noise_rows_dev,
            raw_normals_dev, map, n_noise, rng_seed, rng_round, (int)row0);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

int rb_learner_create(rb_learner_t** out, const rb_learner_config_t* cfg, float* online_params_dev,
                      float* target_params_dev, float* grads_dev, float* online_noise_dev, float* target_noise_dev,
                      uint64_t seed) {
  RB_REQUIRE(out && cfg && online_params_dev && target_params_dev && grads_dev && online_noise_dev && target_noise_dev,
             "rb_learner_create: NULL argument");
  Layout L;
  int rc = make_layout(cfg, &L);
  if (rc != RB_OK) return rc;
  RbOpts opt;
  rc = rb_opts_parse(getenv("RB_OPTS"), &opt);
  if (rc != RB_OK) return rc;
  rb_learner* l = new (std::nothrow) rb_learner();
  if (!l) { rb_set_error("rb_learner_create: host OOM"); return RB_ERR_OOM; }
  memset(l, 0, sizeof(*l));
  l->cfg = *cfg; l->L = L; l->opt = opt;
  l->p_online = online_params_dev; l->p_target = target_params_dev; l->grads = grads_dev;
  l->n_online = online_noise_dev; l->n_target = target_noise_dev;
  l->seed = seed; l->noise_epoch = 0;
  l->world = 1;
  {
    const int64_t seg[6] = {(int64_t)L.B * L.NZ, (int64_t)L.B * 2 * L.H, (int64_t)L.B * 2 * L.H, (int64_t)L.B * L.F, L.n_noise, L.h_mu};
    int64_t off = 0;
    for (int i = 0; i < 6; ++i) { l->fact_off[i] = off; off = align64(off + seg[i]); }
    l->fact_stride = off;
  }
  l->n_eff = cfg->multi_step; l->discount = cfg->discount;
  l->gamma_n = (float)pow(cfg->discount, (double)cfg->multi_step);
  l->delta_z = (float)(((double)cfg->v_max - (double)cfg->v_min) / (double)(cfg->atoms - 1));
  const int B = L.B, NI = 3 * B;
  l->caps = plan_caps(L, l->opt);
#define RB_ALLOC(ptr, count)                                                                         \
  do {                                                                                               \
    hipError_t e_ = rb_dev_malloc((void**)&(ptr), (size_t)(count) * 4);                                  \
    if (e_ != hipSuccess) {                                                                          \
      rb_set_error("rb_learner_create: hipMalloc(%lld B) failed: %s", (long long)(count) * 4, hipGetErrorString(e_)); \
      rb_learner_destroy(l);                                                                         \
      return RB_ERR_OOM;                                                                             \
    }                                                                                                \
  } while (0)
  for (int i = 0; i < L.nconv; ++i) {
    const ConvLayer& c = L.conv[i];
    RB_ALLOC(l->act[i], (int64_t)NI * c.cout * c.P());
    RB_ALLOC(l->dact[i], (int64_t)B * c.cout * c.P());
    {
      int64_t slices = l->caps.ws[i];
      if (slices < (int64_t)B * 5) slices = (int64_t)B * 5;   // LDS weight-grad kernels: B images x <=5 row chunks
      RB_ALLOC(l->dw_part[i], slices * c.cout * (c.K() + 1));
    }
    if (l->caps.wT[i]) {
      const int tmax = (c.ks + c.s - 1) / c.s;
      const int64_t n = (int64_t)c.s * c.s * (c.cin / 32) * (rb_div_up(c.cout * tmax * tmax, 16) * 16) * 32;
      RB_ALLOC(l->conv_wT[i], n);
      RB_HIP_TRY(hipMemset(l->conv_wT[i], 0, (size_t)n * 4));
    }
  }
  l->rows_cap = NI;
  RB_ALLOC(l->hpart, (int64_t)l->caps.hs * NI * 2 * L.H);
  RB_ALLOC(l->h, (int64_t)NI * 2 * L.H);
  RB_ALLOC(l->feat_b, (int64_t)NI * (L.F + 16));
  RB_ALLOC(l->h_b, (int64_t)NI * (2 * L.H + 16));
  RB_ALLOC(l->logits, (int64_t)NI * L.NZ);
  RB_ALLOC(l->dlogits, (int64_t)B * L.NZ);
  RB_ALLOC(l->dlogitsT, (int64_t)B * L.NZ);
  RB_ALLOC(l->dh, (int64_t)B * 2 * L.H);
  RB_ALLOC(l->dhT, (int64_t)B * 2 * L.H);
  RB_ALLOC(l->dfeat_part, (int64_t)l->caps.xs * B * L.F);
  RB_ALLOC(l->log_ps_a, (int64_t)B * L.Z);
  RB_ALLOC(l->pns_a, (int64_t)B * L.Z);
  RB_ALLOC(l->m, (int64_t)B * L.Z);
  RB_ALLOC(l->a_star, (int64_t)B);
  RB_ALLOC(l->support, (int64_t)L.Z);
  RB_ALLOC(l->zero_noise, L.n_noise);
  RB_ALLOC(l->noise_snap, L.n_noise);
  RB_ALLOC(l->norm_part, RB_NORM_PART_SLOTS);
  RB_ALLOC(l->noise_ctr, 4);
  RB_ALLOC(l->status_copy, 4);
  RB_ALLOC(l->adam_args_dev, (sizeof(ClipAdamArgs) + 3) / 4);
  RB_ALLOC(l->act_ctr, 6 * RB_FAN_SHARDS * RB_FAN_STRIDE + 32);
#undef RB_ALLOC
  RB_HIP_TRY(hipMemset(l->act_ctr, 0, (6 * RB_FAN_SHARDS * RB_FAN_STRIDE + 32) * 4));
  if (l->opt.spec_draw) {
    hipError_t e = rb_dev_malloc((void**)&l->go_flag, 64);
    if (e != hipSuccess) { rb_set_error("rb_learner_create: hipMalloc failed: %s", hipGetErrorString(e)); rb_learner_destroy(l); return RB_ERR_OOM; }
    RB_HIP_TRY(hipMemset(l->go_flag, 0, 64));
  }
#if defined(RB_HOST_INTERP)
  l->n_cu = 8;
#else
  {
    int dev = 0, cus = 0;
    RB_HIP_TRY(hipGetDevice(&dev));
    RB_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    l->n_cu = cus;
  }
#endif
  if (l->caps.gemm_ws) {
    // split-K scratch of k_fc_gemm_fwd: tiles * S <= n_cu whenever S > 1, one 128 x 128 partial tile each
    hipError_t e = rb_dev_malloc((void**)&l->gemm_part, (size_t)l->n_cu * RB_TG_T * RB_TG_T * 4);
    if (e == hipSuccess) e = rb_dev_malloc((void**)&l->gemm_ctr, 1024 * 4);
    if (e != hipSuccess) { rb_set_error("rb_learner_create: hipMalloc failed: %s", hipGetErrorString(e)); rb_learner_destroy(l); return RB_ERR_OOM; }
    RB_HIP_TRY(hipMemset(l->gemm_ctr, 0, 1024 * 4));
  }
  RB_HIP_TRY(hipMemset(l->noise_ctr, 0, 16));
  RB_HIP_TRY(hipMemset(l->status_copy, 0, 16));
  float sup[RB_MAX_ATOMS];
  linspace_f32(cfg->v_min, cfg->v_max, L.Z, sup);
  RB_HIP_TRY(hipMemcpy(l->support, sup, L.Z * sizeof(float), hipMemcpyHostToDevice));
  RB_HIP_TRY(hipMemset(l->zero_noise, 0, L.n_noise * sizeof(float)));
  RB_HIP_TRY(hipMemset(l->hpart, 0, (size_t)l->caps.hs * NI * 2 * L.H * 4));
  // the learn call writes the tensors' elements only; k_sumsq (sumsq_pass) and the optimiser pass sweep the whole flat buffer, the
  // alignment padding between the tensors included: it is cleared here, once, and stays zero (include/rainbow_hip.h)
  RB_HIP_TRY(hipMemset(grads_dev, 0, (size_t)L.n_params * 4));
  {
    const int rc = upload_noise_jobs(l);
    if (rc != RB_OK) return rc;
  }
  *out = l;
  return RB_OK;
}

// The learn step's launch sequence; every "which kernel, what grid" is a plan of learner_plan.h, taken by the
// launch function it names.
static int learn_impl(rb_learner_t* l, const ImgSrc& src, const uint8_t* states_dev, const int64_t* actions_dev,
                      const float* returns_dev, const float* nonterminals_dev, const float* weights_dev, float* loss_dev,
                      hipStream_t stream) {
  const Layout& L = l->L;
  const int B = L.B;
  l->cur_src = src;
  const NetPtrs on = net_ptrs(L, l->p_online, l->n_online);
  const NetPtrs tg = net_ptrs(L, l->p_target, l->n_target);
  int rc = forward(l, 2 * B, B, src, on, tg, stream);
  if (rc != RB_OK) return rc;
  {
    // tenant workgroups of the head launch: the conv input-gradient kernels' weight operand of this step (conv_dx.h rb_conv_wt_block)
    const HeadPlan hp = plan_head(plan_in(l));
    HeadTenants tn;
    memset(&tn, 0, sizeof(tn));
    for (int j = 0; j < hp.n_jobs; ++j) {
      const int layer = hp.job_layer[j];
      const ConvLayer& c = L.conv[layer];
      const int tmax = (c.ks + c.s - 1) / c.s;
      tn.job[j] = ConvWtJob{on.conv_w[layer], l->conv_wT[layer], c.cin, c.cout, c.ks, c.s, (int)rb_div_up(c.cout * tmax * tmax, 16) * 16,
                            hp.job_t16[j]};
    }
    if (hp.n_jobs == 1) tn.job[1] = tn.job[0];
    tn.per_job = hp.per_job;
    const dim3 hgrid(hp.blocks), hblock((unsigned)(64 * hp.waves));
#define RB_HEAD_ARGS B, L.Z, L.A, (const float*)l->logits, actions_dev, returns_dev, nonterminals_dev, weights_dev, (const float*)l->support, \
    l->cfg.v_min, l->cfg.v_max, l->gamma_n, l->delta_z, l->log_ps_a, l->pns_a, l->m, l->a_star, loss_dev, l->dlogits, l->step_ctr,          \
    l->batch_status, l->status_copy, l->dlogitsT, tn
    switch (hp.ZI) {
      case 1: RB_LAUNCH_T("head:k_head", k_head<1>, hgrid, hblock, stream, RB_HEAD_ARGS); break;
      case 2: RB_LAUNCH_T("head:k_head", k_head<2>, hgrid, hblock, stream, RB_HEAD_ARGS); break;
      default: RB_LAUNCH_T("head:k_head", k_head<4>, hgrid, hblock, stream, RB_HEAD_ARGS); break;
    }
#undef RB_HEAD_ARGS
  }
  RB_LAUNCH_CHECK();

  // ---- backward (online net, images [0,B)): the two noisy layers, then the conv stack
  const bool exch = plan_in(l).exch;     // replica exchange: the conv gradients are stored into this rank's block as well
  if ((rc = fc_backward(l, on, loss_dev, stream)) != RB_OK) return rc;
  if (l->caps.fast_conv) {
    for (int layer = L.nconv - 1; layer > 0; --layer)                 // the input-gradient chain first ...
      if ((rc = conv_dx(l, layer, stream)) != RB_OK) return rc;
    if ((rc = conv_dw_all(l, stream)) != RB_OK) return rc;            // ... then every weight gradient in one launch
  } else {
    for (int layer = L.nconv - 1; layer >= 0; --layer) {
      if ((rc = conv_dw_gemm(l, layer, states_dev, stream)) != RB_OK) return rc;
      if ((rc = conv_dx(l, layer, stream)) != RB_OK) return rc;
    }
  }
  {   // one fixed-order reduction of every conv layer's split slices into the gradient buffer
    ReduceAllArgs ra;
    int64_t off = 0;
    for (int layer = 0; layer < L.nconv; ++layer) {
      const ConvLayer& c = L.conv[layer];
      ra.layer[layer] = ReduceLayer{l->dw_part[layer], l->grads + L.conv_w[layer], l->grads + L.conv_b[layer],
                                    l->dw_slices[layer], c.cout, c.K(), off};
      off += (int64_t)c.cout * (c.K() + 1);
    }
    ra.n_layers = L.nconv; ra.total = off;
    ra.sq_part = l->norm_slots > 0 ? l->norm_part + l->norm_conv_base : nullptr;
    ra.grads_base = l->grads;
    ra.copy_base = exch ? l->fact_local + l->fact_off[5] : nullptr;
    ra.snap_src = nullptr; ra.snap_dst = nullptr; ra.snap_n = 0; ra.snap_clear = nullptr;
    if (l->sigma_implicit) { ra.snap_src = l->n_online; ra.snap_dst = l->noise_snap; ra.snap_n = (int)L.n_noise; ra.snap_clear = l->status_copy + 2; }
    RB_LAUNCH(k_reduce_conv_dw_all, dim3(plan_conv_reduce_blocks(L, ra.snap_n > 0)), dim3(64), stream, ra);
    RB_LAUNCH_CHECK();
  }
  // with a record ring set (rb_learner_set_stats): this call's rb_step_stats_t, one launch (learn_stats.h); otherwise nothing
  return learn_step_stats(l, loss_dev, weights_dev, returns_dev, nonterminals_dev, stream);
}

int rb_learner_learn(rb_learner_t* l, const uint8_t* states_dev, const uint8_t* next_states_dev,
                     const int64_t* actions_dev, const float* returns_dev, const float* nonterminals_dev,
                     const float* weights_dev, float* loss_dev, rb_stream_t stream_) {
  RB_REQUIRE(l && states_dev && next_states_dev && actions_dev && returns_dev && nonterminals_dev && weights_dev && loss_dev,
             "rb_learner_learn: NULL argument");
  RB_FLUSH_UPDATE(l, stream_);
  ImgSrc src;
  memset(&src, 0, sizeof(src));
  src.u8_states = states_dev; src.u8_next = next_states_dev; src.B = l->L.B;
  return learn_impl(l, src, states_dev, actions_dev, returns_dev, nonterminals_dev, weights_dev, loss_dev, (hipStream_t)stream_);
}

int rb_learner_learn_windows(rb_learner_t* l, const uint8_t* frames_dev, const int32_t* windows_dev, int32_t window_len,
                             const int64_t* actions_dev, const float* returns_dev, const float* nonterminals_dev,
                             const float* weights_dev, float* loss_dev, rb_stream_t stream_) {
  RB_REQUIRE(l && frames_dev && windows_dev && actions_dev && returns_dev && nonterminals_dev && weights_dev && loss_dev,
             "rb_learner_learn_windows: NULL argument");
  RB_FLUSH_UPDATE(l, stream_);
  RB_REQUIRE(window_len == l->L.hist + l->cfg.multi_step, "rb_learner_learn_windows: window_len must be history + multi_step");
  if (!l->caps.fast_conv) {
    rb_set_error("rb_learner_learn_windows: zero-copy frames need the LDS conv kernels (history <= 4); gather the stacks and "
                 "call rb_learner_learn instead");
    return RB_ERR_STATE;
  }
  ImgSrc src;
  memset(&src, 0, sizeof(src));
  src.B = l->L.B; src.ring = frames_dev; src.win = windows_dev; src.win_len = window_len; src.n_step = l->n_eff;
  return learn_impl(l, src, nullptr, actions_dev, returns_dev, nonterminals_dev, weights_dev, loss_dev, (hipStream_t)stream_);
}

static int train_step_impl(rb_learner_t* l, const rb_train_step_t* a, rb_comm_t* comm, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr && a != nullptr && a->replay != nullptr, "rb_learner_train_step: NULL argument");
  {   // this call draws the batch itself: targets built from another horizon or discount than the replay's returns are refused
    int32_t rn = 0;
    double rg = 0.0;
    rb_replay_horizon(a->replay, &rn, &rg);
    RB_REQUIRE(rn == l->n_eff && rg == l->discount, "rb_learner_train_step: the replay's horizon and discount (%d, %.17g) differ from "
               "the learner's (%d, %.17g): call rb_replay_set_horizon and rb_learner_set_horizon with the same values", (int)rn, rg,
               (int)l->n_eff, l->discount);
  }
  // the previous call's optimiser pass, if it was left pending, rides in this call's sampler launch (adam_body.h)
  rb_noise_job_t hosted_job;
  const rb_noise_job_t* job = a->noise_job;
  bool hosted = false;
  if (l->adam_pending) {
    if (job != nullptr && attach_pending_pass(l, job, a->batch, &hosted_job)) {
      job = &hosted_job;
      hosted = true;
    } else {
      const int rc = flush_update(l, (hipStream_t)stream);
      if (rc != RB_OK) return rc;
    }
  }
  // the early draw (RB_OPTS spec_draw=1; off by default): from the SECOND consecutive call with the same replay, batch, beta and
  // buffers — and nothing else having touched the replay in between — this call's write-back and the next call's draw leave for the
  // replay's stream behind the head kernel.  main.py's loop never meets the condition (it appends and anneals beta between learn
  // calls, main.py:157,161): this is for append-free loops only (a PER benchmark, bench.py).  Never under stream capture: the pair
  // would be launched now, outside the graph, waiting for a flag the captured kernels only store on replay.
  {
    auto& t = l->ts_last;
    const bool capturing = l->opt.spec_draw && rb_stream_capturing(stream);
    const bool same = !capturing && t.valid && t.replay == a->replay && t.batch == a->batch && t.max_attempts == a->max_attempts &&
                      t.beta == a->priority_weight &&
                      t.tree_idx == a->tree_idx_dev && t.actions == a->actions_dev && t.returns == a->returns_dev &&
                      t.nonterm == a->nonterminals_dev && t.weights == a->weights_dev && t.mut_after == rb_replay_mutations(a->replay);
    t.streak = same ? t.streak + 1 : 0;
    l->spec_now = (l->opt.spec_draw && t.streak >= 1 && comm == nullptr && a->noise_job != nullptr && a->batch <= 256 && l->caps.fast_fc &&
                   l->sink == a->replay && l->sink_idx == a->tree_idx_dev && rb_replay_spec_allowed(a->replay)) ? 1 : 0;
    if (l->spec_now) {
      rb_spec_request& q = l->spec_req;
      memset(&q, 0, sizeof(q));
      q.batch = a->batch; q.priority_weight = a->priority_weight; q.max_attempts = a->max_attempts;
      q.tree_idx = a->tree_idx_dev; q.actions = a->actions_dev; q.returns = a->returns_dev; q.nonterminals = a->nonterminals_dev;
      q.weights = a->weights_dev;
    }
    if (l->opt.spec_draw && !capturing) rb_replay_spec_arm_accept(a->replay);     // only THIS caller reads the table of the accepted draw
  }
  int rc = rb_replay_sample_fused_noise(a->replay, a->batch, a->priority_weight, nullptr, a->max_attempts, a->tree_idx_dev, nullptr,
                                        nullptr, a->actions_dev, a->returns_dev, a->nonterminals_dev, a->weights_dev,
                                        job, stream);
  if (rc != RB_OK) { l->spec_now = 0; return rc; }
  if (hosted) l->adam_pending = 0;
  // (the window table of THIS draw: an accepted early draw filled the replay's other table)
  rc = rb_learner_learn_windows(l, a->frames_dev, rb_replay_current_windows(a->replay), a->window_len, a->actions_dev, a->returns_dev,
                                a->nonterminals_dev, a->weights_dev, a->loss_dev, stream);
  l->spec_now = 0;
  {
    auto& t = l->ts_last;
    t.replay = a->replay; t.batch = a->batch; t.max_attempts = a->max_attempts; t.beta = a->priority_weight; t.tree_idx = a->tree_idx_dev;
    t.actions = a->actions_dev; t.returns = a->returns_dev; t.nonterm = a->nonterminals_dev; t.weights = a->weights_dev;
    t.mut_after = rb_replay_mutations(a->replay); t.valid = rc == RB_OK ? 1 : 0;
  }
  if (rc != RB_OK) return rc;
  if (comm) {      // replicas: the factor all-gather + the finishing launch between backward and clip (agent.py:96-97)
    rc = rb_learner_exchange_rccl(l, comm, stream);
    if (rc != RB_OK) return rc;
  }
  return clip_adam_impl(l, a->max_norm, a->exp_avg_dev, a->exp_avg_sq_dev, a->lr, a->beta1, a->beta2, a->eps, a->step,
                        a->norm_dev, (hipStream_t)stream, (l->flags & RB_LEARNER_DEFER_UPDATE) != 0);
}

int rb_learner_train_step(rb_learner_t* l, const rb_train_step_t* a, rb_stream_t stream) {
  return train_step_impl(l, a, nullptr, stream);
}
int rb_learner_train_step_dist(rb_learner_t* l, const rb_train_step_t* a, rb_comm_t* comm, rb_stream_t stream) {
  RB_REQUIRE(comm != nullptr, "rb_learner_train_step_dist: NULL communicator");
  return train_step_impl(l, a, comm, stream);
}
// The effective horizon and discount of the targets (include/rainbow_hip.h): host state read when a step is launched, no launch here.
int rb_learner_set_horizon(rb_learner_t* l, int32_t n_eff, double discount) {
  RB_REQUIRE(l != nullptr, "rb_learner_set_horizon: NULL handle");
  RB_REQUIRE(n_eff >= 1 && n_eff <= l->cfg.multi_step, "rb_learner_set_horizon: n_eff must be in [1, %d] (the multi_step the learner "
             "was created with), got %d", (int)l->cfg.multi_step, (int)n_eff);
  RB_REQUIRE(discount > 0.0 && discount <= 1.0, "rb_learner_set_horizon: discount must be in (0, 1], got %g", discount);   // (also NaN)
  l->n_eff = n_eff; l->discount = discount;
  l->gamma_n = (float)pow(discount, (double)n_eff);
  return RB_OK;
}

int rb_learner_get_horizon(rb_learner_t* l, int32_t* n_eff, double* discount) {
  RB_REQUIRE(l && n_eff && discount, "rb_learner_get_horizon: NULL argument");
  *n_eff = l->n_eff; *discount = l->discount;
  return RB_OK;
}

int rb_learner_set_step_counter(rb_learner_t* l, int64_t* step_dev) {
  RB_REQUIRE(l != nullptr, "rb_learner_set_step_counter: NULL handle");
  l->step_ctr = reinterpret_cast<long long*>(step_dev);
  return RB_OK;
}

int rb_learner_set_flags(rb_learner_t* l, int32_t flags) {
  RB_REQUIRE(l != nullptr, "rb_learner_set_flags: NULL handle");
  RB_REQUIRE((flags & ~(RB_LEARNER_FUSE_FC_H_DW | RB_LEARNER_WRITE_FUSED_GRADS | RB_LEARNER_DEFER_UPDATE | RB_LEARNER_IMPLICIT_SIGMA)) == 0,
             "rb_learner_set_flags: unknown flag bits");
  l->flags = flags;
  return RB_OK;
}

int rb_learner_get_rng(rb_learner_t* l, uint64_t* seed, uint64_t* epoch, rb_stream_t stream) {
  RB_REQUIRE(l && seed && epoch, "rb_learner_get_rng: NULL argument");
  RB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long e = 0;
  RB_HIP_TRY(hipMemcpy(&e, l->noise_ctr, sizeof(e), hipMemcpyDeviceToHost));
  *seed = l->seed; *epoch = (uint64_t)e;
  return RB_OK;
}

int rb_learner_set_rng(rb_learner_t* l, uint64_t seed, uint64_t epoch, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_set_rng: NULL handle");
  RB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  const unsigned long long e[2] = {(unsigned long long)epoch, 0ull};
  RB_HIP_TRY(hipMemcpy(l->noise_ctr, e, sizeof(e), hipMemcpyHostToDevice));
  l->seed = seed;
  return upload_noise_jobs(l);   // the device copies of the noise jobs carry the seed (callers re-query the host copy)
}

int rb_learner_set_priority_sink(rb_learner_t* l, rb_replay_t* replay, const int64_t* tree_idx_dev) {
  RB_REQUIRE(l != nullptr, "rb_learner_set_priority_sink: NULL handle");
  RB_REQUIRE((replay == nullptr) == (tree_idx_dev == nullptr), "rb_learner_set_priority_sink: pass both or neither");
  l->sink = replay;
  l->sink_idx = tree_idx_dev;
  l->batch_status = nullptr;
  if (replay) {
    ReplayView v;
    double omega;
    if (rb_replay_internal_view(replay, &v, &omega) != RB_OK) { rb_set_error("rb_learner_set_priority_sink: bad replay handle"); return RB_ERR_INVALID; }
    l->batch_status = &v.hdr->last_status;
  }
  return RB_OK;
}

int rb_learner_zero_copy_ok(rb_learner_t* l) {
  return (l && l->caps.fast_conv) ? 1 : 0;
}

int rb_learner_priority_written(rb_learner_t* l) {
  return (l && l->sink_done) ? 1 : 0;
}

int rb_learner_grads_modified(rb_learner_t* l) {
  RB_REQUIRE(l != nullptr, "rb_learner_grads_modified: NULL handle");
  if (l->dw_deferred) {
    rb_set_error("rb_learner_grads_modified: the hidden layer's weight gradient was not materialised (RB_LEARNER_FUSE_FC_H_DW)");
    return RB_ERR_STATE;
  }
  if (l->sigma_implicit) {
    rb_set_error("rb_learner_grads_modified: the hidden layer's sigma gradient was not materialised (RB_LEARNER_IMPLICIT_SIGMA): "
                 "call rb_learner_flush before reading or modifying grads_dev");
    return RB_ERR_STATE;
  }
  l->norm_slots = 0;
  return RB_OK;
}

int rb_learner_sync_target(rb_learner_t* l, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_sync_target: NULL handle");
  RB_FLUSH_UPDATE(l, stream);
  // load_state_dict copies parameters AND the epsilon buffers (agent.py:102-103)
  RB_HIP_TRY(hipMemcpyAsync(l->p_target, l->p_online, (size_t)l->L.n_params * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  RB_HIP_TRY(hipMemcpyAsync(l->n_target, l->n_online, (size_t)l->L.n_noise * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return RB_OK;
}

#if defined(RB_STAMP)
// RB_STAMP builds: what the runtime says about the residency of the first layer's forward kernels
int rb_debug_occupancy(void) {
  int a = 0, b = 0;
  typedef CfgC1 C;
  constexpr int T16_THREADS = 64 * ConvFwdWaves<C::KMAX, C::PCH, true>::NWV;
  const void* t16 = (const void*)(k_conv_fwd_t16<C::G, C::NT, C::PR, C::KMAX, true, C::PCH>);
  hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, t16, T16_THREADS, 0);
  hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, (const void*)(k_conv_fwd_lds<C::G, C::NT, C::PR, C::KMAX, true, C::PCH>), RB_CONV_THREADS, 0);
  hipFuncAttributes fa;
  hipFuncGetAttributes(&fa, t16);
  printf("occupancy API: conv1 t16 (%d threads) %d blocks/CU, conv1 lds (%d threads) %d; t16: regs %d lds %zu maxThreads %d\n", T16_THREADS, a, RB_CONV_THREADS, b, fa.numRegs, fa.sharedSizeBytes, fa.maxThreadsPerBlock);
  return a;
}
#endif
int rb_learner_debug_read(rb_learner_t* l, int32_t what, void* out_dev, rb_stream_t stream) {
  RB_REQUIRE(l && out_dev, "rb_learner_debug_read: NULL argument");
  if (what < 5) RB_FLUSH_UPDATE(l, stream);      // (5 .. 8 are activations of the last learn call: a pending optimiser pass stays pending)
  const Layout& L = l->L;
  const void* src = nullptr;
  size_t bytes = 0;
  switch (what) {
    case 0: src = l->log_ps_a; bytes = (size_t)L.B * L.Z * 4; break;
    case 1: src = l->m; bytes = (size_t)L.B * L.Z * 4; break;
    case 2: src = l->a_star; bytes = (size_t)L.B * 4; break;
    case 3: src = l->pns_a; bytes = (size_t)L.B * L.Z * 4; break;
    case 4: src = l->logits; bytes = (size_t)3 * L.B * L.NZ * 4; break;
    case 5: src = l->h; bytes = (size_t)L.B * 2 * L.H * 4; break;     // hidden activations of the differentiated forward (rows [0, B))
    case 6: case 7: case 8: {                                         // conv layer (what - 6)'s activations of the same forward: [B][cout][P]
      const int layer = what - 6;
      RB_REQUIRE(layer < L.nconv, "rb_learner_debug_read: the network has no such conv layer");
      src = l->act[layer]; bytes = (size_t)L.B * L.conv[layer].cout * L.conv[layer].oh * L.conv[layer].oh * 4;
      break;
    }
    default: rb_set_error("rb_learner_debug_read: unknown selector %d", what); return RB_ERR_INVALID;
  }
  RB_HIP_TRY(hipMemcpyAsync(out_dev, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return RB_OK;
}

}  // extern "C"
