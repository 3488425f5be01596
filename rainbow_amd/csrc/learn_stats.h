// learn_stats.h — device-side read-outs of the learn step: k_step_stats (one rb_step_stats_t per call, into the caller's ring
// or into the record rb_learner_eval_loss was given), its launch, and the two entry points.  Included by learner.hip only, after
// head.h (k_head) and fc_dispatch.h (forward).
//
// The kernel reads what the step has produced anyway — log p(s_t, a_t), the projected target m, the per-sample loss, the draw's
// weights / returns / nonterminals, the norm partials — and writes 64 bytes.  Rows are spread over workgroups (RB_STATS_ROWS each,
// one wave per row at a time: batch 1024 x 256 atoms is 64 workgroups, not one CU); a row's three sums over atoms are wave
// reductions in double; the last workgroup to arrive (stats_common.h) folds the rows in double: thread t its contiguous run of
// ceil(B / 256) rows in row order, then a wave per sum adds the 256 runs (four per lane, then a fixed butterfly).  No step of
// that depends on the schedule.
#pragma once
#include "learner_internal.h"
#include "stats_common.h"

#define RB_STATS_ROWS 16          // rows per workgroup
#define RB_STATS_THREADS 256      // the norm's summation order (below) holds at exactly this many threads
static_assert(sizeof(rb_step_stats_t) == 64, "rb_step_stats_t is documented as 64 bytes");

struct StepStatsArgs {
  const float* log_ps_a;          // [B][Z]
  const float* m;                 // [B][Z]
  const float* support;           // [Z]
  const float* loss;              // [B]
  const float* weights;           // [B]
  const float* returns;           // [B]
  const float* nonterminals;      // [B]
  const long long* step_ctr;      // NULL: step = -1
  const int32_t* status;          // NULL: status = 0
  const float* norm_part;         // [norm_slots]
  int norm_slots;                 // 0: grad_norm = NaN
  int B, Z;
  double* rows;                   // [3][B] scratch: q, q_target, entropy of every row
  unsigned* ticket;
  rb_step_stats_t* ring;
  int capacity;
  long long* count;               // NULL: ring[0] is written, nothing is counted (rb_learner_eval_loss)
};

__global__ __launch_bounds__(RB_STATS_THREADS) void k_step_stats(StepStatsArgs a) {
  __shared__ float s_red[16];
  __shared__ int s_flag;
  __shared__ double s_run[9][RB_STATS_THREADS];
  __shared__ float s_max[RB_STATS_THREADS];
  __shared__ double s_tot[9];
  const int t = (int)threadIdx.x, lane = rb_lane(), wave = rb_wave();
  const int B = a.B, Z = a.Z;
  const int r0 = (int)blockIdx.x * RB_STATS_ROWS;
  const int r1 = r0 + RB_STATS_ROWS < B ? r0 + RB_STATS_ROWS : B;
  for (int b = r0 + wave; b < r1; b += RB_STATS_THREADS / 64) {      // wave-uniform
    double q = 0.0, qt = 0.0, en = 0.0;
    for (int z = lane; z < Z; z += 64) {
      const float lp = a.log_ps_a[(int64_t)b * Z + z];
      const float p = expf(lp);
      const double s = (double)a.support[z];
      q += s * (double)p;
      qt += s * (double)a.m[(int64_t)b * Z + z];
      if (p > 0.0f) en -= (double)p * (double)lp;                    // (p == 0: the term's limit, not 0 * -inf)
    }
    q = rb_wave_sum_f64(q); qt = rb_wave_sum_f64(qt); en = rb_wave_sum_f64(en);
    if (lane == 0) { rb_pub_f64(a.rows + b, q); rb_pub_f64(a.rows + B + b, qt); rb_pub_f64(a.rows + 2 * B + b, en); }
  }
  if (!rb_last_arrival(a.ticket, gridDim.x, &s_flag)) return;
  // ---- the fold (one workgroup): sums 0 loss, 1 w * loss, 2 w, 3 q, 4 q_target, 5 |q_target - q|, 6 entropy, 7 return, 8 terminal rows
  const int per = (B + RB_STATS_THREADS - 1) / RB_STATS_THREADS;
  double acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.0;
  float mx = -INFINITY;
  for (int b = t * per; b < (t + 1) * per && b < B; ++b) {
    const float lo = a.loss[b], w = a.weights[b];
    const double q = rb_sub_f64(a.rows + b), qt = rb_sub_f64(a.rows + B + b);
    acc[0] += (double)lo; acc[1] += (double)w * (double)lo; acc[2] += (double)w;
    acc[3] += q; acc[4] += qt; acc[5] += fabs(qt - q); acc[6] += rb_sub_f64(a.rows + 2 * B + b);
    acc[7] += (double)a.returns[b]; acc[8] += a.nonterminals[b] == 0.0f ? 1.0 : 0.0;
    mx = fmaxf(mx, lo);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) s_run[k][t] = acc[k];
  s_max[t] = mx;
  // the norm, in the order of the optimiser pass (adam_body.h's hosted prologue and k_clip_adam): thread t adds partials t, t + 256,
  // ... in index order, then rb_block_sum, then sqrtf
  float nsq = 0.0f;
  for (int i = t; i < a.norm_slots; i += RB_STATS_THREADS) nsq += a.norm_part[i];
  nsq = rb_block_sum(nsq, s_red);                                    // (its barriers also publish s_run / s_max)
  // the 256 runs of each sum: one wave per sum, lane l adds runs 4 l .. 4 l + 3 left to right, then the fixed butterfly over the
  // lanes (a lone thread walking the 256 LDS words one dependent read at a time took ~16 us: profiles/diag_bench.txt)
  float vmax = -INFINITY;
  for (int item = wave; item < 10; item += RB_STATS_THREADS / 64) {   // wave-uniform; item 9 is the maximum
    if (item < 9) {
      const double* r = s_run[item] + 4 * lane;
      const double tot = rb_wave_sum_f64(((r[0] + r[1]) + r[2]) + r[3]);
      if (lane == 0) s_tot[item] = tot;
    } else {
      const float* r = s_max + 4 * lane;
      vmax = rb_wave_max(fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3])));
    }
  }
  __syncthreads();
  if (wave == 9 % (RB_STATS_THREADS / 64) && lane == 0) s_max[0] = vmax;   // (behind the barrier: every wave has read its runs)
  __syncthreads();
  if (t != 0) return;
  const double n = (double)B;
  rb_step_stats_t rec;
  rec.step = a.step_ctr ? (int64_t)*a.step_ctr : (int64_t)-1;
  rec.batch = B;
  rec.status = a.status ? *a.status : 0;
  rec.loss_mean = (float)(s_tot[0] / n); rec.loss_max = s_max[0];
  rec.wloss_mean = (float)(s_tot[1] / n); rec.weight_mean = (float)(s_tot[2] / n);
  rec.q_mean = (float)(s_tot[3] / n); rec.q_target_mean = (float)(s_tot[4] / n); rec.td_abs_mean = (float)(s_tot[5] / n);
  rec.entropy_mean = (float)(s_tot[6] / n); rec.return_mean = (float)(s_tot[7] / n); rec.terminal_frac = (float)(s_tot[8] / n);
  rec.grad_norm = a.norm_slots > 0 ? sqrtf(nsq) : NAN;
  rec.reserved = 0.0f;
  long long slot = 0;
  if (a.count) slot = *a.count % (long long)a.capacity;
  a.ring[slot] = rec;
  if (a.count) *a.count = *a.count + 1;
}

// scratch of the read-outs, allocated by whichever entry point needs it first (synchronises once: include/rainbow_hip.h)
// Each buffer is checked on its own and becomes the handle's only once it is filled: a call that fails half way leaves what it
// allocated to rb_learner_destroy and the next call allocates only what is still missing.
static int stats_scratch(rb_learner* l) {
  const int B = l->L.B;
  if (!l->stats_ticket) {
    unsigned* p = nullptr;
    RB_HIP_TRY(rb_dev_malloc((void**)&p, 64));
    if (hipMemset(p, 0, 64) != hipSuccess) { rb_dev_free(p); rb_set_error("rb_learner: clearing the stats ticket failed"); return RB_ERR_HIP; }
    l->stats_ticket = p;
  }
  if (!l->ones) {
    float* p = nullptr;
    RB_HIP_TRY(rb_dev_malloc((void**)&p, (size_t)B * 4));
    float one[1024];
    for (int i = 0; i < B; ++i) one[i] = 1.0f;
    if (hipMemcpy(p, one, (size_t)B * 4, hipMemcpyHostToDevice) != hipSuccess) { rb_dev_free(p); rb_set_error("rb_learner: filling the unit weights failed"); return RB_ERR_HIP; }
    l->ones = p;
  }
  if (!l->stats_rows) RB_HIP_TRY(rb_dev_malloc((void**)&l->stats_rows, (size_t)3 * B * sizeof(double)));
  return RB_OK;
}

// One record of the step whose buffers are in the handle right now.  ring != NULL.
static int launch_step_stats(rb_learner* l, const float* loss_dev, const float* weights, const float* returns, const float* nonterminals,
                             const long long* step_ctr, const int32_t* status, int norm_slots, rb_step_stats_t* ring, int capacity,
                             long long* count, hipStream_t stream) {
  const Layout& L = l->L;
  StepStatsArgs a;
  a.log_ps_a = l->log_ps_a; a.m = l->m; a.support = l->support; a.loss = loss_dev;
  a.weights = weights; a.returns = returns; a.nonterminals = nonterminals;
  a.step_ctr = step_ctr; a.status = status; a.norm_part = l->norm_part; a.norm_slots = norm_slots;
  a.B = L.B; a.Z = L.Z; a.rows = l->stats_rows; a.ticket = l->stats_ticket;
  a.ring = ring; a.capacity = capacity; a.count = count;
  RB_LAUNCH(k_step_stats, dim3((unsigned)rb_div_up(L.B, RB_STATS_ROWS)), dim3(RB_STATS_THREADS), stream, a);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

// the record of a learn call (learn_impl's last launch); nothing without a ring
static int learn_step_stats(rb_learner* l, const float* loss_dev, const float* weights, const float* returns, const float* nonterminals,
                            hipStream_t stream) {
  if (!l->stats_ring) return RB_OK;
  return launch_step_stats(l, loss_dev, weights, returns, nonterminals, l->step_ctr, l->status_copy, l->norm_slots, l->stats_ring,
                           l->stats_cap, l->stats_count, stream);
}

extern "C" {

int rb_learner_set_stats(rb_learner_t* l, rb_step_stats_t* ring_dev, int32_t capacity, int64_t* count_dev) {
  RB_REQUIRE(l != nullptr, "rb_learner_set_stats: NULL handle");
  RB_REQUIRE((ring_dev == nullptr) == (count_dev == nullptr), "rb_learner_set_stats: pass ring_dev and count_dev, or neither");
  if (!ring_dev) { l->stats_ring = nullptr; l->stats_count = nullptr; l->stats_cap = 0; return RB_OK; }
  RB_REQUIRE(capacity >= 1, "rb_learner_set_stats: capacity must be >= 1, got %d", (int)capacity);
  const int rc = stats_scratch(l);
  if (rc != RB_OK) return rc;
  l->stats_ring = ring_dev; l->stats_cap = capacity; l->stats_count = reinterpret_cast<long long*>(count_dev);
  return RB_OK;
}

int rb_learner_eval_loss(rb_learner_t* l, const uint8_t* states_dev, const uint8_t* next_states_dev, const int64_t* actions_dev,
                         const float* returns_dev, const float* nonterminals_dev, float* loss_dev, rb_step_stats_t* stats_out_dev,
                         rb_stream_t stream_) {
  RB_REQUIRE(l != nullptr, "rb_learner_eval_loss: NULL handle (l)");
  RB_REQUIRE(states_dev != nullptr, "rb_learner_eval_loss: NULL states_dev");
  RB_REQUIRE(next_states_dev != nullptr, "rb_learner_eval_loss: NULL next_states_dev");
  RB_REQUIRE(actions_dev != nullptr, "rb_learner_eval_loss: NULL actions_dev");
  RB_REQUIRE(returns_dev != nullptr, "rb_learner_eval_loss: NULL returns_dev");
  RB_REQUIRE(nonterminals_dev != nullptr, "rb_learner_eval_loss: NULL nonterminals_dev");
  RB_REQUIRE(loss_dev != nullptr, "rb_learner_eval_loss: NULL loss_dev");
  hipStream_t stream = (hipStream_t)stream_;
  RB_FLUSH_UPDATE(l, stream);
  if (l->exch_pending) {
    rb_set_error("rb_learner_eval_loss: the gradients of the last learn call still wait for rb_learner_finish_grads, which reads the "
                 "activations this call overwrites");
    return RB_ERR_STATE;
  }
  if (l->dw_deferred) {
    rb_set_error("rb_learner_eval_loss: the last learn call left the hidden layer's weight gradient to the fused optimiser pass "
                 "(RB_LEARNER_FUSE_FC_H_DW), which reads the activations this call overwrites; call rb_learner_clip_adam first");
    return RB_ERR_STATE;
  }
  int rc = stats_scratch(l);
  if (rc != RB_OK) return rc;
  const Layout& L = l->L;
  const int B = L.B;
  ImgSrc src;
  memset(&src, 0, sizeof(src));
  src.u8_states = states_dev; src.u8_next = next_states_dev; src.B = B;
  const NetPtrs on = net_ptrs(L, l->p_online, l->zero_noise);      // eval mode, both networks (model.py:46)
  const NetPtrs tg = net_ptrs(L, l->p_target, l->zero_noise);
  if ((rc = forward(l, 2 * B, B, src, on, tg, stream)) != RB_OK) return rc;
  {
    const HeadPlan hp = plan_head(plan_in(l));
    HeadTenants tn;
    memset(&tn, 0, sizeof(tn));                                     // no tenants: the backward they prepare does not follow
    const dim3 hgrid((unsigned)B), hblock((unsigned)(64 * hp.waves));
#define RB_EVAL_HEAD_ARGS B, L.Z, L.A, (const float*)l->logits, actions_dev, returns_dev, nonterminals_dev, (const float*)l->ones,          \
    (const float*)l->support, l->cfg.v_min, l->cfg.v_max, l->gamma_n, l->delta_z, l->log_ps_a, l->pns_a, l->m, l->a_star, loss_dev,       \
    l->dlogits, (long long*)nullptr, (const int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr, tn
    switch (hp.ZI) {
      case 1: RB_LAUNCH_T("head:k_head", k_head<1>, hgrid, hblock, stream, RB_EVAL_HEAD_ARGS); break;
      case 2: RB_LAUNCH_T("head:k_head", k_head<2>, hgrid, hblock, stream, RB_EVAL_HEAD_ARGS); break;
      default: RB_LAUNCH_T("head:k_head", k_head<4>, hgrid, hblock, stream, RB_EVAL_HEAD_ARGS); break;
    }
#undef RB_EVAL_HEAD_ARGS
    RB_LAUNCH_CHECK();
  }
  if (!stats_out_dev) return RB_OK;
  return launch_step_stats(l, loss_dev, l->ones, returns_dev, nonterminals_dev, nullptr, nullptr, 0, stats_out_dev, 1, nullptr, stream);
}

}  // extern "C"
