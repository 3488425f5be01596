// optimizer_host.h — host side of the optimiser: the global-norm clip, clip + Adam in one pass, the pending pass
// (RB_LEARNER_DEFER_UPDATE) and its hosting, the implicit sigma gradient.  Included by learner.hip only, after adam_kernels.h and
// grad_finish.h (the kernels) and fc_dispatch.h (fc_dw_plan).
#pragma once
#include "learner_plan.h"

static int materialize_sigma(rb_learner* l, hipStream_t stream) {
  if (!l->sigma_implicit) return RB_OK;
  const Layout& L = l->L;
  const NetPtrs sn = net_ptrs(L, l->p_online, l->noise_snap);
  const int64_t len4 = (int64_t)2 * L.H * L.F / 4;
  RB_LAUNCH(k_materialize_sigma, dim3((unsigned)rb_div_up(len4, 256 * 4)), dim3(256), stream, l->grads, L.h_mu / 4, len4, L.F / 4, L.H,
            sn.h_eout, sn.h_ein, (const int32_t*)(l->status_copy + 2));
  RB_LAUNCH_CHECK();
  l->sigma_implicit = 0;
  return RB_OK;
}

// The pending optimiser pass (RB_LEARNER_DEFER_UPDATE) as a launch of its own: every entry point that reads or writes
// parameters, moments, gradients or the norm calls this first — only the next rb_learner_train_step hosts it instead.
static int flush_update(rb_learner* l, hipStream_t stream) {
  if (!l->adam_pending) return RB_OK;
  FusedDwAdamArgs f;
  memset(&f, 0, sizeof(f));
  ClipAdamArgs a = l->adam_args_host;
  int blocks = l->adam_blocks;
  if (a.pair_len4 > 0) {        // the pending pass forms the sigma gradient itself: the hosted body as a launch of its own
    const int rc = rb_launch_adam_pending(l->adam_args_dev, blocks, stream, a.t != nullptr);      // (its arguments are in device memory already)
    if (rc != RB_OK) return rc;
    l->adam_pending = 0;
    return RB_OK;
  }
  if (a.t) RB_LAUNCH_T("clip_adam:k_clip_adam", (k_clip_adam<4, true, false, true>), dim3((unsigned)blocks), dim3(256), stream, a, f);
  else RB_LAUNCH_T("clip_adam:k_clip_adam", (k_clip_adam<4, true, false>), dim3((unsigned)blocks), dim3(256), stream, a, f);
  RB_LAUNCH_CHECK();
  l->adam_pending = 0;
  return RB_OK;
}

// The gradient's sum of squares when no learn call left partials (it came from the fallback path or was modified since — an
// all-reduce): ONE pass over it into norm_part.  *nparts = the partials written.
static int sumsq_pass(rb_learner* l, hipStream_t stream, int* nparts) {
  const int64_t n = l->L.n_params;
  *nparts = plan_sumsq_blocks(n);
  RB_LAUNCH(k_sumsq, dim3((unsigned)*nparts), dim3(256), stream, (const float*)l->grads, n, l->norm_part);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

// job_out = job_in + the pending optimiser pass as extra workgroups of the sampler launch that takes the job (adam_body.h); a plain
// copy (returns false) when nothing is pending or the launch cannot host it.  The caller clears adam_pending once that launch is out.
static bool attach_pending_pass(rb_learner* l, const rb_noise_job_t* job_in, int32_t batch, rb_noise_job_t* job_out) {
  memcpy(job_out, job_in, sizeof(*job_out));
  if (!l->adam_pending || batch > 256) return false;
  NoiseJob* nj = reinterpret_cast<NoiseJob*>(job_out);
  nj->adam_dev = l->adam_args_dev; nj->adam_blocks = l->adam_blocks;
  nj->adam_ema = l->adam_args_host.t != nullptr ? 1 : 0;
  return true;
}

// One EMA step of the target towards the online parameters as a launch of its own (adam_kernels.h k_target_ema): behind the fused
// tile pass, and rb_learner_target_ema (status = NULL: unconditional).
static int launch_target_ema(rb_learner* l, float tau, const int32_t* status, hipStream_t stream) {
  const int64_t n = l->L.n_params;
  const int64_t n4 = n >> 2;
  RB_LAUNCH_T("clip_adam:k_target_ema", k_target_ema, dim3((unsigned)rb_div_up(n4 > 0 ? n4 : 1, 256 * 4)), dim3(256), stream, l->p_target,
              (const float*)l->p_online, n, tau, status);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

static int clip_adam_impl(rb_learner* l, float max_norm, float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2,
                          double eps, int64_t step, float* norm_dev, hipStream_t stream, bool defer) {
  RB_REQUIRE(exp_avg != nullptr && exp_avg_sq != nullptr, "rb_learner_clip_adam: NULL moment buffer");
  RB_REQUIRE(step >= 1 || (step == 0 && l->step_ctr), "rb_learner_clip_adam: step is 1-based (0 = take it from the device counter set "
             "with rb_learner_set_step_counter)");
  const int64_t n = l->L.n_params;
  int nparts = l->norm_slots;
  if (!(max_norm < INFINITY) && norm_dev == nullptr) {
    nparts = 0;        // plain optimiser.step(): no clip, nobody wants the norm
  } else if (nparts <= 0) {
    const int rcs = sumsq_pass(l, stream, &nparts);
    if (rcs != RB_OK) return rcs;
  }
  l->norm_slots = 0;   // consumed
  ClipAdamArgs a;
  memset(&a, 0, sizeof(a));
  a.p = l->p_online; a.g = l->grads; a.m = exp_avg; a.v = exp_avg_sq; a.n = n;
  a.part = l->norm_part; a.nparts = nparts; a.max_norm = max_norm; a.norm_out = norm_dev;
  // scalars exactly as torch.optim.adam._single_tensor_adam forms them (python doubles, rounded once to f32 by the op)
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  a.w1 = (float)(1.0 - beta1); a.b2 = (float)beta2; a.w2 = (float)(1.0 - beta2);
  a.neg_step_size = (float)(-(lr / bc1)); a.bc2_sqrt = (float)sqrt(bc2); a.eps = (float)eps;
  a.step_dev = step == 0 ? l->step_ctr : nullptr; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2;
  a.batch_status = l->status_copy;        // (k_head's copy of l->batch_status: see status_copy)
  const bool ema = l->target_tau > 0.0f;  // (both fields stay zero otherwise: the argument block, and with it every launch, is today's)
  if (ema && !l->dw_deferred) { a.t = l->p_target; a.tau = l->target_tau; }
  const int64_t n4 = n >> 2;
  // 4 quadruples per thread: measured best of {2, 4, 8} on MI355X (254.3 / 255.6 / 256.6 us per step)
  // write-through stores (same-box A/B 253.7 -> 250.8 us per step) through buffer instructions: offsets are 31-bit
  RB_REQUIRE(n * 4 < (int64_t)0x7fffffff, "rb_learner_clip_adam: the flat parameter buffer must be smaller than 2 GiB");
  FusedDwAdamArgs f;
  memset(&f, 0, sizeof(f));
  a.skip_lo4 = 0; a.skip_len4 = 0;
  if (l->dw_deferred) {
    const Layout& L = l->L;
    const NetPtrs on = net_ptrs(L, l->p_online, l->n_online);
    FcDwPlan hp = fc_dw_plan(l, on, 1, l->dh, l->act[L.nconv - 1], L.B, 0);
    f.dw = hp.a;
    f.mu_off = L.h_mu; f.sigma_off = L.h_sigma;
    f.dw_x = hp.dw_x; f.n_tile_blocks = 2 * hp.dw_x * hp.dw_y;     // two slots per tile: mu, sigma
    f.write_grads = (l->flags & RB_LEARNER_WRITE_FUSED_GRADS) ? 1 : 0;
    a.skip_lo4 = L.h_mu >> 2; a.skip_len4 = (L.h_bmu - L.h_mu) >> 2;
    const unsigned grid = (unsigned)(f.n_tile_blocks + rb_div_up(n4 - a.skip_len4 > 0 ? n4 - a.skip_len4 : 1, 256 * 4));
    RB_LAUNCH_T("clip_adam:k_clip_adam", (k_clip_adam<4, true, true>), dim3(grid), dim3(256), stream, a, f);
    l->dw_deferred = 0;
    if (ema) {      // the tile pass carries no EMA (adam_kernels.h): the stand-alone launch right behind it, same rule, same skip
      RB_LAUNCH_CHECK();
      return launch_target_ema(l, l->target_tau, a.batch_status, stream);
    }
  } else {
    unsigned grid = (unsigned)rb_div_up(n4 > 0 ? n4 : 1, 256 * 4);
    const bool will_defer = defer && a.step_dev != nullptr && a.nparts > 0 && l->adam_args_dev != nullptr;
    if (l->sigma_implicit && will_defer) {
      // the hosted pass updates (mu, sigma) quads of the hidden layer together and forms g_sigma itself (adam_body.h)
      const Layout& L = l->L;
      const NetPtrs sn = net_ptrs(L, l->p_online, l->noise_snap);
      a.pair_mu4 = L.h_mu / 4; a.pair_len4 = (int64_t)2 * L.H * L.F / 4;
      a.pair_f4 = L.F / 4; a.pair_split_row = L.H; a.pair_eout = sn.h_eout; a.pair_ein = sn.h_ein;
      a.pair_clipped = l->status_copy + 2;
      a.hole_lo4 = (unsigned)a.pair_mu4; a.hole4 = (unsigned)(2 * a.pair_len4);
      a.pair_blk0 = (int)rb_div_up(n4 - 2 * a.pair_len4 > 0 ? n4 - 2 * a.pair_len4 : 1, 256 * 4);
      grid = (unsigned)(a.pair_blk0 + rb_div_up(a.pair_len4, 256 * 2));   /* adam_body.h rb_adam_hosted_pairs: 2 pairs per thread */
    } else if (l->sigma_implicit) {
      const int rcm = materialize_sigma(l, stream);
      if (rcm != RB_OK) return rcm;
    }
    if (will_defer) {
      // left pending: the next train_step's sampler launch hosts these workgroups (or flush_update launches them).  The
      // arguments are all step-invariant (the step number and the norm partials live on the device): uploaded on change only
      if (!l->adam_args_valid || memcmp(&a, &l->adam_args_host, sizeof(a)) != 0) {
        RB_LAUNCH(k_store_adam_args, dim3(1), dim3(64), stream, a, l->adam_args_dev);
        RB_LAUNCH_CHECK();
        memcpy(&l->adam_args_host, &a, sizeof(a));
        l->adam_args_valid = 1;
      }
      l->adam_pending = 1;
      l->adam_blocks = (int)grid;
      return RB_OK;
    }
    if (ema) RB_LAUNCH_T("clip_adam:k_clip_adam", (k_clip_adam<4, true, false, true>), dim3(grid), dim3(256), stream, a, f);
    else RB_LAUNCH_T("clip_adam:k_clip_adam", (k_clip_adam<4, true, false>), dim3(grid), dim3(256), stream, a, f);
  }
  RB_LAUNCH_CHECK();
  return RB_OK;
}

extern "C" {

int rb_learner_set_target_tau(rb_learner_t* l, float tau, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_set_target_tau: NULL handle");
  RB_REQUIRE(tau >= 0.0f && tau <= 1.0f, "rb_learner_set_target_tau: tau must be in [0, 1], got %g", (double)tau);
  RB_FLUSH_UPDATE(l, stream);          // a pending pass's device-side arguments carry the old tau: it runs with that one
  l->target_tau = tau;                 // (the next pass's argument block differs: the upload-on-change memcmp picks it up)
  return RB_OK;
}

int rb_learner_target_ema(rb_learner_t* l, float tau, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_target_ema: NULL handle");
  RB_REQUIRE(tau >= 0.0f && tau <= 1.0f, "rb_learner_target_ema: tau must be in [0, 1], got %g", (double)tau);
  RB_FLUSH_UPDATE(l, stream);
  if (tau == 0.0f) return RB_OK;
  return launch_target_ema(l, tau, nullptr, (hipStream_t)stream);
}

int rb_learner_flush(rb_learner_t* l, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_flush: NULL handle");
  const int rc = flush_update(l, (hipStream_t)stream);
  if (rc != RB_OK) return rc;
  return materialize_sigma(l, (hipStream_t)stream);      // (a caller about to read grads_dev: RB_LEARNER_IMPLICIT_SIGMA)
}

// The same hosting for a caller that issues the step's entry points one by one (Agent's eager path, the replica exchange):
// attach fills `job_out` = `job_in` + the pending pass (returns 1) or leaves it a plain copy (0); the caller passes job_out
// to rb_replay_sample_fused_noise and, once that launch is in the stream, calls rb_learner_pending_launched.
int rb_learner_attach_pending(rb_learner_t* l, const rb_noise_job_t* job_in, int32_t batch, rb_noise_job_t* job_out) {
  if (!l || !job_in || !job_out) { rb_set_error("rb_learner_attach_pending: NULL argument"); return RB_ERR_INVALID; }
  return attach_pending_pass(l, job_in, batch, job_out) ? 1 : 0;
}
int rb_learner_pending_launched(rb_learner_t* l) {
  RB_REQUIRE(l != nullptr, "rb_learner_pending_launched: NULL handle");
  l->adam_pending = 0;
  return RB_OK;
}
// TESTS ONLY (not declared in rainbow_hip.h): one optimiser pass over caller-owned buffers of ANY length.  The learner's own
// flat buffers are padded to whole quads and never shorter than a block, so the n % 4 tail, a last block of clamped loads and
// a pair range that ends inside a workgroup are reached only this way.  form 0: k_clip_adam<4, true, false> with the step by
// value (the reference form); form 1: the hosted body as k_adam_pending, its arguments stored to `args_dev` (256 bytes) first,
// the step read from `step_dev`.  `part` holds `nparts` > 0 partial sums of squares.  pair_len4 > 0 (form 1 only): quads
// [pair_mu4, pair_mu4 + pair_len4) are a layer's mu weights, the pair_len4 quads behind them its sigma weights, whose gradient
// the pass forms from pair_eout [rows] and pair_ein [2][4 * pair_f4] (ClipAdamArgs, adam_body.h).
static int debug_adam_pass_impl(int32_t form, float* p, float* g, float* m, float* v, int64_t n, const float* part, int32_t nparts,
                               float max_norm, float* norm_out, const long long* step_dev, int64_t step, double lr, double beta1,
                               double beta2, double eps, const int32_t* batch_status, int64_t pair_mu4, int64_t pair_len4, int32_t pair_f4,
                               int32_t pair_split_row, const float* pair_eout, const float* pair_ein, int32_t* pair_clipped, void* args_dev,
                               float* target, float tau, rb_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RB_REQUIRE(p && g && m && v && part && n >= 0 && n * 4 < (int64_t)0x7fffffff && nparts > 0, "rb_debug_adam_pass: bad buffers");
  RB_REQUIRE(form == 0 ? (step >= 1 && pair_len4 == 0) : (form == 1 && step_dev && args_dev), "rb_debug_adam_pass: bad form");
  static_assert(sizeof(ClipAdamArgs) <= 256, "rb_debug_adam_pass: args_dev is documented as 256 bytes");
  ClipAdamArgs a;
  memset(&a, 0, sizeof(a));
  a.p = p; a.g = g; a.m = m; a.v = v; a.n = n;
  a.part = part; a.nparts = nparts; a.max_norm = max_norm; a.norm_out = norm_out;
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  a.w1 = (float)(1.0 - beta1); a.b2 = (float)beta2; a.w2 = (float)(1.0 - beta2);
  a.neg_step_size = (float)(-(lr / bc1)); a.bc2_sqrt = (float)sqrt(bc2); a.eps = (float)eps;
  a.step_dev = form == 1 ? step_dev : nullptr; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2;
  a.batch_status = batch_status;
  a.t = target; a.tau = target ? tau : 0.0f;
  const int64_t n4 = n >> 2;
  unsigned grid = (unsigned)rb_div_up(n4 > 0 ? n4 : 1, 256 * 4);
  if (form == 0) {
    FusedDwAdamArgs f;
    memset(&f, 0, sizeof(f));
    if (target) RB_LAUNCH((k_clip_adam<4, true, false, true>), dim3(grid), dim3(256), stream, a, f);
    else RB_LAUNCH((k_clip_adam<4, true, false>), dim3(grid), dim3(256), stream, a, f);
    RB_LAUNCH_CHECK();
    return RB_OK;
  }
  if (pair_len4 > 0) {
    RB_REQUIRE(pair_mu4 >= 0 && pair_mu4 + 2 * pair_len4 <= n4 && pair_f4 > 0 && pair_len4 % pair_f4 == 0 && pair_eout && pair_ein,
               "rb_debug_adam_pass: bad pair range");
    a.pair_mu4 = pair_mu4; a.pair_len4 = pair_len4; a.pair_f4 = pair_f4; a.pair_split_row = pair_split_row;
    a.pair_eout = pair_eout; a.pair_ein = pair_ein; a.pair_clipped = pair_clipped;
    a.hole_lo4 = (unsigned)pair_mu4; a.hole4 = (unsigned)(2 * pair_len4);
    a.pair_blk0 = (int)rb_div_up(n4 - 2 * pair_len4 > 0 ? n4 - 2 * pair_len4 : 1, 256 * 4);
    grid = (unsigned)(a.pair_blk0 + rb_div_up(pair_len4, 256 * 2));
  }
  RB_LAUNCH(k_store_adam_args, dim3(1), dim3(64), stream, a, reinterpret_cast<ClipAdamArgs*>(args_dev));
  RB_LAUNCH_CHECK();
  return rb_launch_adam_pending(reinterpret_cast<const ClipAdamArgs*>(args_dev), (int)grid, stream, target != nullptr);
}

int rb_debug_adam_pass(int32_t form, float* p, float* g, float* m, float* v, int64_t n, const float* part, int32_t nparts,
                       float max_norm, float* norm_out, const long long* step_dev, int64_t step, double lr, double beta1,
                       double beta2, double eps, const int32_t* batch_status, int64_t pair_mu4, int64_t pair_len4, int32_t pair_f4,
                       int32_t pair_split_row, const float* pair_eout, const float* pair_ein, int32_t* pair_clipped, void* args_dev,
                       rb_stream_t stream_) {
  return debug_adam_pass_impl(form, p, g, m, v, n, part, nparts, max_norm, norm_out, step_dev, step, lr, beta1, beta2, eps, batch_status,
                              pair_mu4, pair_len4, pair_f4, pair_split_row, pair_eout, pair_ein, pair_clipped, args_dev, nullptr, 0.0f, stream_);
}
// TESTS ONLY as well: the same pass with a target attached (`target` [n], tau in (0, 1]): the EMA instantiations — form 0
// k_clip_adam<4, true, false, true>, form 1 k_adam_pending_ema — at the lengths only rb_debug_adam_pass reaches.
int rb_debug_adam_pass_ema(int32_t form, float* p, float* g, float* m, float* v, int64_t n, const float* part, int32_t nparts,
                           float max_norm, float* norm_out, const long long* step_dev, int64_t step, double lr, double beta1,
                           double beta2, double eps, const int32_t* batch_status, int64_t pair_mu4, int64_t pair_len4, int32_t pair_f4,
                           int32_t pair_split_row, const float* pair_eout, const float* pair_ein, int32_t* pair_clipped, void* args_dev,
                           float* target, float tau, rb_stream_t stream_) {
  RB_REQUIRE(target != nullptr && tau > 0.0f && tau <= 1.0f, "rb_debug_adam_pass_ema: needs a target and tau in (0, 1]");
  return debug_adam_pass_impl(form, p, g, m, v, n, part, nparts, max_norm, norm_out, step_dev, step, lr, beta1, beta2, eps, batch_status,
                              pair_mu4, pair_len4, pair_f4, pair_split_row, pair_eout, pair_ein, pair_clipped, args_dev, target, tau, stream_);
}

// rb_learner_clip_adam that leaves the pass pending when the handle's flags say so (RB_LEARNER_DEFER_UPDATE) and it can
// (step = 0 with a device step counter, norm partials from the learn call); otherwise exactly rb_learner_clip_adam.
int rb_learner_clip_adam_deferred(rb_learner_t* l, float max_norm, float* exp_avg, float* exp_avg_sq, double lr, double beta1,
                                  double beta2, double eps, int64_t step, float* norm_dev, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_clip_adam_deferred: NULL handle");
  const int rc = flush_update(l, (hipStream_t)stream);
  if (rc != RB_OK) return rc;
  return clip_adam_impl(l, max_norm, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, norm_dev, (hipStream_t)stream,
                        (l->flags & RB_LEARNER_DEFER_UPDATE) != 0);
}

int rb_learner_clip_grad(rb_learner_t* l, float max_norm, float* norm_dev, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_clip_grad: NULL handle");
  RB_FLUSH_UPDATE(l, stream);
  RB_MATERIALIZE_SIGMA(l, stream);
  if (l->dw_deferred) {
    rb_set_error("rb_learner_clip_grad: the last learn call left the hidden layer's weight gradient to the fused optimiser "
                 "pass (RB_LEARNER_FUSE_FC_H_DW); call rb_learner_clip_adam, or clear the flag before learning");
    return RB_ERR_STATE;
  }
  const int64_t n = l->L.n_params;
  int nblocks = plan_sumsq_blocks(n);
  int nparts = l->norm_slots;
  if (nparts > 0) {
    // every block of the scale kernel re-sums the partial list (same order everywhere): keep that redundant work small.
    // The scale loop itself only runs when the norm exceeds max_norm.
    if (nblocks > 256) nblocks = 256;
  } else {
    const int rcs = sumsq_pass(l, (hipStream_t)stream, &nparts);
    if (rcs != RB_OK) return rcs;
  }
  l->norm_slots = 0;   // consumed
  RB_LAUNCH(k_clip_scale, dim3((unsigned)nblocks), dim3(256), stream, l->grads, n, (const float*)l->norm_part, nparts,
            max_norm, norm_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

int rb_learner_clip_adam(rb_learner_t* l, float max_norm, float* exp_avg, float* exp_avg_sq, double lr, double beta1,
                         double beta2, double eps, int64_t step, float* norm_dev, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_clip_adam: NULL handle");
  const int rc = flush_update(l, (hipStream_t)stream);
  if (rc != RB_OK) return rc;
  return clip_adam_impl(l, max_norm, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, norm_dev, (hipStream_t)stream, false);
}

}  // extern "C"
