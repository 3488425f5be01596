// act_host.h — host side of Agent.act / evaluate_q: the act path of one state (act_path.h k_act_fused, as one launch or as one
// launch per phase) and the batched forward + head (act_batch_run, behind the three rb_learner_act_batch* entry points).
// Included by learner.hip only, after fc_dispatch.h (forward, fc_rows_fwd, nl_h / nl_z) and head.h (k_head_act, k_head_act_eps).
#pragma once
#include "learner_internal.h"

// Output rows per workgroup of each conv layer on the act path (act_conv.h rb_act_conv_unit): at most RB_ACT_MAXPOS
// positions, and the rows' input patch within RB_ACT_LDS floats.  false = a layer the act path does not cover (no row fits, or a
// filter beyond RB_ACT_KMAX taps).  rb_debug_launch_plan prints the same numbers (act_path rg=).
static bool act_conv_rows(const Layout& L, int rg[3]) {
  rg[0] = rg[1] = rg[2] = 0;
  for (int layer = 0; layer < L.nconv; ++layer) {
    const ConvLayer& c = L.conv[layer];
    int r = RB_ACT_MAXPOS / c.oh;
    if (r > c.oh) r = c.oh;
    while (r >= 1 && (int64_t)c.cin * ((r - 1) * c.s + c.ks) * c.ih > RB_ACT_LDS) --r;
    if (r < 1 || c.K() > RB_ACT_KMAX) return false;
    rg[layer] = r;
  }
  return true;
}
// Whether rb_learner_act runs the act path at all (RB_OPTS generic=1 / 2 clears fast_fc); otherwise the training forward
static bool act_path_covers(const Layout& L, const LearnerCaps& caps, int rg[3]) {
  rg[0] = rg[1] = rg[2] = 0;
  if (!caps.fast_fc || (L.F & 3) || (L.H & 3)) return false;
  return act_conv_rows(L, rg);
}

// One state through the act path (act_path.h).  RB_ERR_STATE (without touching the error string) = geometry not
// covered, the caller falls back to the training kernels.
// Returns 1 (the forward AND the head ran, in either launch form, and wrote head_action_out / head_q_out), or an error.
static int act_forward_single(rb_learner* l, const float* state_dev, const NetPtrs& on, int noisy, hipStream_t stream,
                              int32_t* head_action_out, float* head_q_out) {
  const Layout& L = l->L;
  int rg[3];
  if (!act_path_covers(L, l->caps, rg)) return RB_ERR_STATE;            // RB_OPTS generic=1 / 2 also lands here
  ActFusedArgs f;
  memset(&f, 0, sizeof(f));
  const float* x = state_dev;
  for (int layer = 0; layer < L.nconv; ++layer) {
    const ConvLayer& c = L.conv[layer];
    ActConvArgs& a = f.conv[layer];
    a.x = x; a.w = on.conv_w[layer]; a.bias = on.conv_b[layer]; a.y = l->act[layer];
    a.cin = c.cin; a.cout = c.cout; a.KS = c.ks; a.S = c.s; a.IH = c.ih; a.OH = c.oh; a.RG = rg[layer];
    x = l->act[layer];
  }
  f.nconv = L.nconv;
  ActFcArgs& h = f.h;
  h.x = x; h.w = nl_h(on); h.K = L.F; h.n_rows = 2 * L.H; h.split_row = L.H; h.x_off1 = 0; h.ein_off1 = L.F;
  h.out = l->h; h.relu = 1; h.mu_only = noisy ? 0 : 1;
  ActFcArgs& z = f.z;
  z.x = l->h; z.w = nl_z(on); z.K = L.H; z.n_rows = L.NZ; z.split_row = L.Z; z.x_off1 = L.H; z.ein_off1 = L.H;
  z.out = l->logits; z.relu = 0; z.mu_only = noisy ? 0 : 1;
  f.Z = L.Z; f.A = L.A; f.logits = l->logits; f.support = l->support; f.action_out = head_action_out; f.q_out = head_q_out;
  f.ctr = l->act_ctr; f.err = l->act_ctr + 6 * RB_FAN_SHARDS * RB_FAN_STRIDE;
  int G = (l->n_cu < 256 ? l->n_cu : 256) / RB_FAN_SHARDS * RB_FAN_SHARDS;       // a multiple of the counter shards
  if (G < RB_FAN_SHARDS) G = RB_FAN_SHARDS;
  // (a captured launch would replay a stale launch number; the host interpreter runs workgroups one after the other, so an
  // in-launch wait could never be met)
  bool one_launch = l->opt.act_fused != 0 && !rb_stream_capturing(stream);
#if defined(RB_HOST_INTERP)
  one_launch = false;
#endif
  if (one_launch) {
    // ONE persistent launch: G workgroups, one per CU, all resident — the in-launch waits need that
    f.phase_lo = 0; f.phase_hi = 6; f.epoch = l->act_epoch + 1;        // (counted below, once the launch is in the stream)
    const int hq = (int)rb_div_up(L.F, 256);
    if (hq <= 3) { RB_LAUNCH_T("act:k_act_fused", k_act_fused<3>, dim3((unsigned)G), dim3(256), stream, f); }
    else if (hq <= 13) { RB_LAUNCH_T("act:k_act_fused", k_act_fused<13>, dim3((unsigned)G), dim3(256), stream, f); }
    else { RB_LAUNCH_T("act:k_act_fused", k_act_fused<0>, dim3((unsigned)G), dim3(256), stream, f); }
    RB_LAUNCH_CHECK();
    ++l->act_epoch;       // only a launch that went out advances the monotonic arrival targets (a refused one signalled nothing)
    return 1;
  }
  // One launch per phase: the same kernel, the same units in the same order, the stream orders the phases.  With phase_hi -
  // phase_lo == 1 a launch of k_act_fused is complete and dependency-free:
  //   - `fused` is false, so nothing is prefetched;
  //   - prev == -1, so nothing waits;
  //   - phase + 1 == phase_hi, so nothing signals (act_epoch is not advanced);
  //   - epoch == 0 switches off the head's error-word check;
  //   - ctr and err are never dereferenced.
  for (int ph = 0; ph < 6; ++ph) {
    if (ph < 3 && ph >= L.nconv) continue;
    f.phase_lo = ph; f.phase_hi = ph + 1; f.epoch = 0;
    RB_LAUNCH(k_act_fused<0>, dim3((unsigned)G), dim3(256), stream, f);
    RB_LAUNCH_CHECK();
  }
  return 1;
}

extern "C" {

int rb_learner_act(rb_learner_t* l, const float* state_dev, int32_t noisy, int32_t* action_dev, float* q_dev,
                   rb_stream_t stream) {
  RB_REQUIRE(l && state_dev, "rb_learner_act: NULL argument");
  RB_FLUSH_UPDATE(l, stream);
  const Layout& L = l->L;
  ImgSrc src;
  memset(&src, 0, sizeof(src));
  src.f32 = state_dev; src.B = 1;
  const NetPtrs on = net_ptrs(L, l->p_online, noisy ? l->n_online : l->zero_noise);
  int rc = act_forward_single(l, state_dev, on, noisy, (hipStream_t)stream, action_dev, q_dev);
  if (rc == 1) return RB_OK;                                                          // the act path, head included
  if (rc == RB_ERR_STATE) rc = forward(l, 1, 0, src, on, on, (hipStream_t)stream);   // geometry outside the act path:
  if (rc != RB_OK) return rc;                                                         // the training forward, then the head
  RB_LAUNCH(k_head_act, dim3(1), dim3(256), stream, L.Z, L.A, (const float*)l->logits, 0, (const float*)l->support,
            action_dev, q_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

// rb_learner_act + waiting for its result on the host, in one call (include/rainbow_hip.h): the action word is preset, the launch
// goes out, and the pinned word is polled HERE — a compiled loop sees the head's store within tens of nanoseconds, a Python loop
// over a numpy scalar within a microsecond or two, and the caller saves the interpreter's share of a 43 us act().
int rb_learner_act_wait(rb_learner_t* l, const float* state_dev, int32_t noisy, int32_t* action_pinned, float* q_pinned,
                        int32_t* action_out, float* q_out, rb_stream_t stream) {
  RB_REQUIRE(l && state_dev && action_pinned && q_pinned, "rb_learner_act_wait: NULL argument");
  constexpr int32_t PENDING = -7;
  int attempts = 0;
  for (;;) {
    *(volatile int32_t*)action_pinned = PENDING;
    const int rc = rb_learner_act(l, state_dev, noisy, action_pinned, q_pinned, stream);
    if (rc != RB_OK) return rc;
#if !defined(RB_HOST_INTERP)
    bool seen = false;
    for (long spin = 0; spin < 4000000L; ++spin) {           // ~10 ms of polling, then the stream is synchronised instead
      if (*(volatile int32_t*)action_pinned != PENDING) { seen = true; break; }
    }
    if (!seen) RB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
#endif
    int32_t a = *(volatile int32_t*)action_pinned;
#if !defined(RB_HOST_INTERP)
    if (a < 0) {                                             // an error code (or a torn view): the final word after a synchronise
      RB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
      a = *(volatile int32_t*)action_pinned;
    }
#endif
    if (a >= 0) {
      if (action_out) *action_out = a;
      if (q_out) *q_out = *(volatile float*)q_pinned;        // (the head stores q, fences, then the action)
      return RB_OK;
    }
    // the one-launch path reported an expired in-launch wait of THAT launch (its workgroups were not co-resident); the failure is
    // tagged with the launch number, so the next launch starts clean: once more, then give up
    if (++attempts >= 2) {
      rb_set_error("rb_learner_act_wait: the one-launch act path reported an expired in-launch wait twice (action %d); "
                   "RB_OPTS=act_fused=0 selects one launch per phase", (int)a);
      return RB_ERR_STATE;
    }
  }
}

}  // extern "C"

// (re)allocate one f32 buffer of `count` floats; `who` names the entry point in the message
static int regrow_f32(float** p, int64_t count, const char* who) {
  if (*p) rb_dev_free(*p);
  *p = nullptr;
  hipError_t e = rb_dev_malloc((void**)p, (size_t)count * 4);
  if (e != hipSuccess) { rb_set_error("%s: hipMalloc(%lld B) failed: %s", who, (long long)count * 4, hipGetErrorString(e)); return RB_ERR_OOM; }
  return RB_OK;
}

// The forward buffers are sized for the learn step's 3B images; batched evaluation (test.py:38-39 over a 500-state
// validation memory) may ask for more rows: grow them (synchronising; happens once per size).
static int ensure_rows(rb_learner* l, int rows) {
  if (rows <= l->rows_cap) return RB_OK;
  const Layout& L = l->L;
  RB_HIP_TRY(hipDeviceSynchronize());
  const char* who = "rb_learner_act_batch";
  int rc;
  for (int i = 0; i < L.nconv; ++i)
    if ((rc = regrow_f32(&l->act[i], (int64_t)rows * L.conv[i].cout * L.conv[i].P(), who)) != RB_OK) return rc;
  if ((rc = regrow_f32(&l->hpart, (int64_t)l->caps.hs * rows * 2 * L.H, who)) != RB_OK) return rc;
  if ((rc = regrow_f32(&l->h, (int64_t)rows * 2 * L.H, who)) != RB_OK) return rc;
  if ((rc = regrow_f32(&l->feat_b, (int64_t)rows * (L.F + 16), who)) != RB_OK) return rc;
  if ((rc = regrow_f32(&l->h_b, (int64_t)rows * (2 * L.H + 16), who)) != RB_OK) return rc;
  if ((rc = regrow_f32(&l->logits, (int64_t)rows * L.NZ, who)) != RB_OK) return rc;
  RB_HIP_TRY(hipMemset(l->hpart, 0, (size_t)l->caps.hs * rows * 2 * L.H * 4));
  l->rows_cap = rows;
  return RB_OK;
}

// The scaled-activation buffers of the per-row-noise path live beside the forward buffers: grown on demand (synchronising; once per size)
static int ensure_rows_scaled(rb_learner* l, int rows) {
  if (rows <= l->rows_s_cap) return RB_OK;
  const Layout& L = l->L;
  if (l->feat_s || l->h_s) RB_HIP_TRY(hipDeviceSynchronize());   // (a launch in flight may still read what is freed below)
  l->rows_s_cap = 0;
  int rc;
  if ((rc = regrow_f32(&l->feat_s, (int64_t)rows * (2 * L.F + 16), "rb_learner_act_batch_rows")) != RB_OK) return rc;
  if ((rc = regrow_f32(&l->h_s, (int64_t)rows * (2 * L.H + 16), "rb_learner_act_batch_rows")) != RB_OK) return rc;
  l->rows_s_cap = rows;
  return RB_OK;
}

// One batched forward + head: what the three rb_learner_act_batch* entry points below ask for, after their own argument checks.
struct ActBatchReq {
  const float* states;        // f32 [n][history][84][84]
  int n, noisy;
  const float* noise_rows;    // non-NULL: row i's noisy layers run under noise row i (fc_rows_fwd); `noisy` is not read
  bool eps;                   // the e-greedy draw in the head (k_head_act_eps) with the five values below
  float epsilon;
  uint64_t rng_seed, rng_round;
  int row0;
  uint8_t* explored;
  int32_t* actions;
  float* q;
};
static int act_batch_run(rb_learner* l, const ActBatchReq& r, hipStream_t stream) {
  RB_FLUSH_UPDATE(l, stream);
  const Layout& L = l->L;
  const int n = r.n;
  int rc = ensure_rows(l, n);
  if (rc != RB_OK) return rc;
  ImgSrc src;
  memset(&src, 0, sizeof(src));
  src.f32 = r.states; src.B = n;
  if (r.noise_rows) {
    const ActRowsPlan p = plan_act_rows(plan_in(l), n);
    if (p.kernel != ACT_ROWS_GENERIC && (rc = ensure_rows_scaled(l, n)) != RB_OK) return rc;
    const NetPtrs on = net_ptrs(L, l->p_online, l->zero_noise);     // (the conv layers carry no noise)
    for (int layer = 0; layer < L.nconv; ++layer)
      if ((rc = conv_fwd(l, layer, n, 0, src, on, on, stream)) != RB_OK) return rc;
    rc = fc_rows_fwd(l, p, n, r.noise_rows, on, stream);
  } else {
    const NetPtrs on = net_ptrs(L, l->p_online, r.noisy ? l->n_online : l->zero_noise);
    rc = forward(l, n, 0, src, on, on, stream);                     // the training kernels: n images share every weight read
  }
  if (rc != RB_OK) return rc;
  if (r.eps) {
    RB_LAUNCH(k_head_act_eps, dim3((unsigned)n), dim3(256), stream, L.Z, L.A, (const float*)l->logits, (const float*)l->support, r.epsilon,
              r.rng_seed, r.rng_round, r.row0, r.actions, r.q, r.explored);
  } else {
    RB_LAUNCH(k_head_act, dim3((unsigned)n), dim3(256), stream, L.Z, L.A, (const float*)l->logits, 0, (const float*)l->support,
              r.actions, r.q);
  }
  RB_LAUNCH_CHECK();
  return RB_OK;
}

extern "C" {

int rb_learner_act_batch(rb_learner_t* l, const float* states_dev, int32_t n, int32_t noisy, int32_t* actions_dev,
                         float* q_dev, rb_stream_t stream) {
  RB_REQUIRE(l && states_dev, "rb_learner_act_batch: NULL argument");
  RB_FLUSH_UPDATE(l, stream);     // (this entry has always flushed before its range check; act_batch_run then finds nothing pending)
  RB_REQUIRE(n >= 1 && n <= 4096, "rb_learner_act_batch: n must be in [1, 4096]");
  if (n == 1) return rb_learner_act(l, states_dev, noisy, actions_dev, q_dev, stream);      // the one-launch path
  ActBatchReq r;
  memset(&r, 0, sizeof(r));
  r.states = states_dev; r.n = n; r.noisy = noisy; r.actions = actions_dev; r.q = q_dev;
  return act_batch_run(l, r, (hipStream_t)stream);
}

// rb_learner_act_batch with row i's noisy layers under noise row i (include/rainbow_hip.h; noisy_rows.h has the arithmetic);
// n == 1 runs the rows forward as well
int rb_learner_act_batch_rows(rb_learner_t* l, const float* states_dev, int32_t n, const float* noise_rows_dev, int32_t* actions_dev,
                              float* q_dev, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_act_batch_rows: NULL handle (l)");
  RB_REQUIRE(states_dev != nullptr, "rb_learner_act_batch_rows: NULL states_dev");
  RB_REQUIRE(noise_rows_dev != nullptr, "rb_learner_act_batch_rows: NULL noise_rows_dev");
  RB_REQUIRE(n >= 1 && n <= 256, "rb_learner_act_batch_rows: n must be in [1, 256], got %d", (int)n);
  ActBatchReq r;
  memset(&r, 0, sizeof(r));
  r.states = states_dev; r.n = n; r.noise_rows = noise_rows_dev; r.actions = actions_dev; r.q = q_dev;
  return act_batch_run(l, r, (hipStream_t)stream);
}

// rb_learner_act_batch with the e-greedy draw in the head (include/rainbow_hip.h): the same forward, the same buffers.
int rb_learner_act_batch_eps(rb_learner_t* l, const float* states_dev, int32_t n, int32_t noisy, float epsilon, uint64_t rng_seed,
                             uint64_t rng_round, int32_t row0, int32_t* actions_dev, float* q_dev, uint8_t* explored_dev,
                             rb_stream_t stream) {
  RB_REQUIRE(l && states_dev, "rb_learner_act_batch_eps: NULL argument");
  RB_REQUIRE(actions_dev, "rb_learner_act_batch_eps: NULL actions_dev (the draw is applied to the stored action)");
  RB_REQUIRE(epsilon >= 0.0f, "rb_learner_act_batch_eps: epsilon must be a number >= 0, got %g", (double)epsilon);
  RB_REQUIRE(row0 >= 0, "rb_learner_act_batch_eps: row0 must be >= 0, got %d", (int)row0);
  RB_REQUIRE(n >= 1 && n <= 4096, "rb_learner_act_batch_eps: n must be in [1, 4096]");
  if (n == 1) {
    // the one-launch act path, then one wave that applies the draw of row0 to the action it stored
    const int rc1 = rb_learner_act_batch(l, states_dev, 1, noisy, actions_dev, q_dev, stream);
    if (rc1 != RB_OK) return rc1;
    RB_LAUNCH(k_act_eps_override, dim3(1), dim3(64), stream, l->L.A, epsilon, rng_seed, rng_round, (int)row0, actions_dev, explored_dev);
    RB_LAUNCH_CHECK();
    return RB_OK;
  }
  ActBatchReq r;
  memset(&r, 0, sizeof(r));
  r.states = states_dev; r.n = n; r.noisy = noisy; r.actions = actions_dev; r.q = q_dev;
  r.eps = true; r.epsilon = epsilon; r.rng_seed = rng_seed; r.rng_round = rng_round; r.row0 = row0; r.explored = explored_dev;
  return act_batch_run(l, r, (hipStream_t)stream);
}

}  // extern "C"
