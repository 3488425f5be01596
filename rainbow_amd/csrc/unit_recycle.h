// unit_recycle.h — recycling dormant units (ReDo: Sokar, Agarwal, Castro, Evci, "The Dormant Neuron Phenomenon in Deep RL", ICML
// 2023): per-unit activity of an eval-mode forward, the dormant mask, and the targeted reset — fresh incoming weights, zeroed
// outgoing weights, so that the network's function does not change.  Included by learner.hip only, after param_reset.h
// (reset_table: the initial distributions) and learn_stats.h (the eval-mode forward sequence of rb_learner_eval_loss).  Never on the
// per-step path: three launches of their own, once per thousands of steps.
//
// A UNIT is an output channel of a conv layer or a hidden unit of fc_h_v / fc_h_a; the layers are conv 0 .. nconv - 1, fc_h_v,
// fc_h_a, their units numbered in that order (rb_learner_unit_layout).  Every kernel here runs one workgroup per unit (or per
// layer), finds its layer by a block-uniform walk over the table in its argument block, and sums in double in an order that
// depends on the thread count alone: thread t its elements in index order, a fixed butterfly over the lanes, the waves in order.
//
// The three launches are ordered by the stream; no workgroup waits for another one.
#pragma once
#include "learner_internal.h"

#define RB_REDO_KEY_TAG 0x5245444Full         // "REDO": a key of its own (RB_RESET_KEY_TAG param_reset.h, RB_SHIFT_KEY_TAG replay_shift.h)
#define RB_REDO_MAX_LAYERS 5                  // at most three conv layers and the two streams of the hidden layer
#define RB_REDO_THREADS 256                   // the summation orders below hold at exactly this many threads
#define RB_REDO_MAX_IN 64                     // most units a unit's incoming row reads from (the widest conv layer)

// By value in the kernels' argument blocks: every field is read through the scalar path.
struct RedoLayer {
  int32_t first, units;       // units [first, first + units) of the numbering
  int32_t P;                  // positions per unit in the activation buffer (conv: oh * oh; hidden: 1)
  int32_t in_first, in_per;   // the layer its incoming rows read from: its first unit (-1: the frames), row elements per input unit
  // incoming parameters of unit i: `row` floats at w_off + i * row (and at w2_off + i * row when w2_off >= 0: the sigma twin, a
  // constant), one float at b_off + i (and at b2_off + i)
  int32_t w_off, w2_off, b_off, b2_off, row;
  float w_bound, w2_val, b_bound, b2_val;
  // outgoing parameters of unit i: `o_rows` runs of `o_len` floats, run r at o_off + r * o_stride + i * o_len (<- 0), and the same
  // runs at o2_off (<- o2_val) when o2_off >= 0
  int32_t o_off, o2_off, o_rows, o_len, o_stride;
  float o2_val;
};
struct RedoMap {
  int32_t n_layers, n_units;
  RedoLayer l[RB_REDO_MAX_LAYERS];
};

static int redo_n_layers(const Layout& L) { return L.nconv + 2; }
static int redo_units(const Layout& L, int layer) { return layer < L.nconv ? L.conv[layer].cout : L.H; }

// The table of a layout; the bounds and constants are reset_table's own entries (param_reset.h), taken from it by position.
static void redo_map(const Layout& L, float noisy_std, RedoMap* M) {
  ResetTable T;
  reset_table(L, 0.0f, 0.0f, noisy_std, &T);      // alpha = 0: every tensor has its entry, in rb_learner_param_layout's order
  memset(M, 0, sizeof(*M));
  M->n_layers = redo_n_layers(L);
  int first = 0;
  const int hb = 2 * L.nconv;                     // fc_h_v: mu, sigma, bias_mu, bias_sigma at hb .. hb + 3, fc_h_a at hb + 4 ..
  const int last = L.nconv - 1;
  for (int k = 0; k < M->n_layers; ++k) {
    RedoLayer& r = M->l[k];
    r.first = first; r.units = redo_units(L, k);
    if (k < L.nconv) {
      const ConvLayer& c = L.conv[k];
      r.P = c.P();
      r.in_first = k > 0 ? M->l[k - 1].first : -1; r.in_per = c.ks * c.ks;
      r.w_off = (int32_t)L.conv_w[k]; r.w2_off = -1; r.b_off = (int32_t)L.conv_b[k]; r.b2_off = -1; r.row = c.K();
      r.w_bound = T.d[2 * k].val; r.b_bound = T.d[2 * k + 1].val;
      if (k < last) {                             // the ks'^2 floats at o * K' + i * ks'^2 of every row o of the next layer's weight
        const ConvLayer& n = L.conv[k + 1];
        r.o_off = (int32_t)L.conv_w[k + 1]; r.o2_off = -1; r.o_rows = n.cout; r.o_len = n.ks * n.ks; r.o_stride = n.K();
      } else {                                    // columns [i P, (i + 1) P) of all 2H rows of h_mu and h_sigma
        r.o_off = (int32_t)L.h_mu; r.o2_off = (int32_t)L.h_sigma; r.o_rows = 2 * L.H; r.o_len = c.P(); r.o_stride = L.F;
        r.o2_val = T.d[hb + 1].val;
      }
    } else {
      const int s = k - L.nconv;                  // 0: fc_h_v, 1: fc_h_a
      r.P = 1;
      r.in_first = M->l[last].first; r.in_per = L.conv[last].P();
      r.w_off = (int32_t)(L.h_mu + (int64_t)s * L.H * L.F); r.w2_off = (int32_t)(L.h_sigma + (int64_t)s * L.H * L.F);
      r.b_off = (int32_t)(L.h_bmu + s * L.H); r.b2_off = (int32_t)(L.h_bsigma + s * L.H); r.row = L.F;
      r.w_bound = T.d[hb + 4 * s].val; r.w2_val = T.d[hb + 4 * s + 1].val;
      r.b_bound = T.d[hb + 4 * s + 2].val; r.b2_val = T.d[hb + 4 * s + 3].val;
      // column i of the stream's rows of z_mu / z_sigma: rows [0, Z) for v, [Z, NZ) for a
      const int64_t row0 = s == 0 ? 0 : L.Z;
      r.o_off = (int32_t)(L.z_mu + row0 * L.H); r.o2_off = (int32_t)(L.z_sigma + row0 * L.H);
      r.o_rows = s == 0 ? L.Z : L.A * L.Z; r.o_len = 1; r.o_stride = L.H;
      r.o2_val = T.d[hb + 8 + 4 * s + 1].val;
    }
    first += r.units;
  }
  M->n_units = first;
}

// the sum of a workgroup's 256 doubles: the fixed butterfly inside a wave, then the waves in order (all threads call)
__device__ __forceinline__ double rb_redo_block_sum(double v, double* lds4) {
  v = rb_wave_sum_f64(v);
  __syncthreads();
  if (rb_lane() == 0) lds4[rb_wave()] = v;
  __syncthreads();
  return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

// the layer of unit u: a block-uniform walk
__device__ __forceinline__ int rb_redo_layer_of(const RedoMap& M, int u) {
  int k = 0;
  for (int j = 1; j < M.n_layers; ++j)
    if (u >= M.l[j].first) k = j;
  return k;
}

extern "C" {

// One workgroup per unit.  Unit i of a conv layer: the B rows' P positions at act[b][i][.]; hidden unit j of stream s: h[b][s H + j].
// Wave w takes rows w, w + 4, ..., lane by lane over the positions: neither order depends on the grid.
__global__ __launch_bounds__(RB_REDO_THREADS) void k_unit_activity(RedoMap M, const float* act0, const float* act1, const float* act2,
                                                                  const float* h, int B, int nconv, int H2, int accumulate, double* activity) {
  __shared__ double s_w[4];
  const int u = (int)blockIdx.x;
  const int k = rb_redo_layer_of(M, u);
  const int i = u - M.l[k].first, P = M.l[k].P;
  const int lane = rb_lane(), wave = rb_wave();
  double acc = 0.0;
  if (k < nconv) {                                                    // block-uniform
    const float* a = k == 0 ? act0 : k == 1 ? act1 : act2;
    const int cout = M.l[k].units;
    for (int b = wave; b < B; b += RB_REDO_THREADS / 64) {
      const float* row = a + ((int64_t)b * cout + i) * P;
      for (int p = lane; p < P; p += 64) acc += (double)row[p];
    }
  } else {
    const int col = (k - nconv) * (H2 / 2) + i;
    for (int b = (int)threadIdx.x; b < B; b += RB_REDO_THREADS) acc += (double)h[(int64_t)b * H2 + col];
  }
  const double tot = rb_redo_block_sum(acc, s_w);
  if (threadIdx.x == 0) activity[u] = accumulate ? activity[u] + tot : tot;
}

// One workgroup per layer.  S = the layer's sum (thread t adds units t, t + 256, ... in index order, then the fixed fold); unit i is
// dormant iff activity[i] * N <= tau * S in double.  A NaN makes every comparison it enters false.
__global__ __launch_bounds__(RB_REDO_THREADS) void k_dormant_mask(RedoMap M, const double* activity, double tau, uint8_t* mask,
                                                                 int32_t* counts, float* scores) {
  __shared__ double s_w[4];
  const int k = (int)blockIdx.x;
  const int first = M.l[k].first, N = M.l[k].units;
  const int t = (int)threadIdx.x;
  double acc = 0.0;
  for (int i = t; i < N; i += RB_REDO_THREADS) acc += activity[first + i];
  const double S = rb_redo_block_sum(acc, s_w);
  const double n = (double)N, bar = tau * S;
  double cnt = 0.0;
  for (int i = t; i < N; i += RB_REDO_THREADS) {
    const double a = activity[first + i];
    const bool dormant = a * n <= bar;
    mask[first + i] = dormant ? (uint8_t)1 : (uint8_t)0;
    if (dormant) cnt += 1.0;
    if (scores) scores[first + i] = S == 0.0 ? 0.0f : (float)(a * n / S);
  }
  cnt = rb_redo_block_sum(cnt, s_w);                                  // (whole numbers below 2^53: exact)
  if (t == 0) counts[k] = (int32_t)cnt;
}

}  // extern "C"

struct RedoBufs {
  float *p, *t, *m, *v;       // t, m, v may be NULL
};
__device__ __forceinline__ void rb_redo_put1(const RedoBufs& b, int idx, float x) {
  b.p[idx] = x;
  if (b.t) b.t[idx] = x;
  if (b.m) { b.m[idx] = 0.0f; b.v[idx] = 0.0f; }
}
__device__ __forceinline__ void rb_redo_put4(const RedoBufs& b, int idx, float4 x) {
  rb_st4(b.p + idx, x);
  if (b.t) rb_st4(b.t + idx, x);
  if (b.m) {
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    rb_st4(b.m + idx, z); rb_st4(b.v + idx, z);
  }
}

// Flat elements [lo, lo + n) <- phi: uniform != 0: val * (2u - 1) with u from word e & 3 of rb_philox(key, draw, e >> 2), e the flat
// index; else the constant val.  Where s_in (LDS, may be NULL) marks the element's input unit, (e - lo) / per, as dormant too, the
// element takes out_val, the OUTGOING rule of that unit (zero wins; that unit's workgroup stores the same value).  Thread t takes
// the flat-aligned quads t, t + 256, ... of the range: one Philox call and one 16-byte store per buffer where the quad lies inside
// the range, element by element at its edges.  theta is never read.
__device__ __forceinline__ void rb_redo_fill_row(const RedoBufs& b, uint64_t key, uint64_t draw, int lo, int n, float val, int uniform,
                                                 const uint8_t* s_in, int per, float out_val) {
  if (n <= 0) return;
  const int q1 = (lo + n - 1) >> 2;
  for (int q = (lo >> 2) + (int)threadIdx.x; q <= q1; q += RB_REDO_THREADS) {
    float x[4];
    unsigned in = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[e] = val;
      if ((unsigned)(4 * q + e - lo) < (unsigned)n) in |= 1u << e;
    }
    if (uniform) {
      const rb_philox_out r = rb_philox(key, draw, (uint64_t)q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float un = (float)(r.v[e] >> 8) * 0x1p-24f;
        x[e] = val * (2.0f * un - 1.0f);
      }
    }
    if (s_in) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (((in >> e) & 1u) && s_in[(4 * q + e - lo) / per]) x[e] = out_val;
    }
    if (in == 15u) {
      rb_redo_put4(b, 4 * q, make_float4(x[0], x[1], x[2], x[3]));
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((in >> e) & 1u) rb_redo_put1(b, 4 * q + e, x[e]);
    }
  }
}

// `rows` runs of `len` floats, run r at base + r * stride <- x: 4-byte stores (the runs start at i * P or at a column: unaligned)
__device__ __forceinline__ void rb_redo_fill_runs(const RedoBufs& b, int base, int rows, int len, int stride, float x) {
  const int total = rows * len;
  for (int e = (int)threadIdx.x; e < total; e += RB_REDO_THREADS) {
    const int r = e / len, c = e - r * len;
    rb_redo_put1(b, base + r * stride + c, x);
  }
}

extern "C" {

// One workgroup per unit; a workgroup whose mask byte is 0 returns at once (block-uniform), so the cost follows the number of dormant
// units.  Incoming rows first (phi, or the outgoing value where the input unit is dormant too), then the outgoing runs.  An element
// that is incoming to one dormant unit and outgoing from another is stored by both workgroups, and both store the same value (the
// outgoing one), so their order does not matter.
__global__ __launch_bounds__(RB_REDO_THREADS) void k_recycle_units(RedoMap M, const uint8_t* mask, float* p, float* t, float* m, float* v,
                                                                  uint64_t key, uint64_t draw) {
  __shared__ uint8_t s_in[RB_REDO_MAX_IN];
  const int u = (int)blockIdx.x;
  if (mask[u] == 0) return;                                           // block-uniform
  const int k = rb_redo_layer_of(M, u);
  const RedoLayer& y = M.l[k];
  const int i = u - y.first;
  RedoBufs b;
  b.p = p; b.t = t; b.m = m; b.v = v;
  const int n_in = y.in_first >= 0 ? y.row / y.in_per : 0;            // the input layer's units, at most RB_REDO_MAX_IN (host-checked)
  if ((int)threadIdx.x < n_in) s_in[threadIdx.x] = mask[y.in_first + (int)threadIdx.x];
  __syncthreads();
  const uint8_t* in = n_in > 0 ? s_in : nullptr;
  rb_redo_fill_row(b, key, draw, y.w_off + i * y.row, y.row, y.w_bound, 1, in, y.in_per, 0.0f);
  rb_redo_fill_row(b, key, draw, y.b_off + i, 1, y.b_bound, 1, nullptr, 1, 0.0f);
  if (y.w2_off >= 0) {                                                // the sigma twins: constants (the outgoing value of h_sigma is the same one)
    rb_redo_fill_row(b, key, draw, y.w2_off + i * y.row, y.row, y.w2_val, 0, nullptr, 1, 0.0f);
    rb_redo_fill_row(b, key, draw, y.b2_off + i, 1, y.b2_val, 0, nullptr, 1, 0.0f);
  }
  rb_redo_fill_runs(b, y.o_off + i * y.o_len, y.o_rows, y.o_len, y.o_stride, 0.0f);
  if (y.o2_off >= 0) rb_redo_fill_runs(b, y.o2_off + i * y.o_len, y.o_rows, y.o_len, y.o_stride, y.o2_val);
}

int rb_learner_unit_layout(const rb_learner_config_t* cfg, int32_t* n_layers, int32_t* units_per_layer) {
  Layout L;
  const int rc = make_layout(cfg, &L);
  if (rc != RB_OK) return rc;
  RB_REQUIRE(n_layers != nullptr, "rb_learner_unit_layout: n_layers is NULL");
  *n_layers = redo_n_layers(L);
  if (units_per_layer)
    for (int k = 0; k < RB_REDO_MAX_LAYERS; ++k) units_per_layer[k] = k < redo_n_layers(L) ? redo_units(L, k) : 0;
  return RB_OK;
}

int rb_learner_unit_activity(rb_learner_t* l, const uint8_t* states_dev, int32_t accumulate, double* activity_dev, rb_stream_t stream_) {
  RB_REQUIRE(l != nullptr, "rb_learner_unit_activity: NULL handle (l)");
  RB_REQUIRE(states_dev != nullptr, "rb_learner_unit_activity: NULL states_dev");
  RB_REQUIRE(activity_dev != nullptr, "rb_learner_unit_activity: NULL activity_dev");
  RB_REQUIRE((uintptr_t)activity_dev % 8 == 0, "rb_learner_unit_activity: activity_dev must be 8-byte aligned");
  hipStream_t stream = (hipStream_t)stream_;
  RB_FLUSH_UPDATE(l, stream);
  if (l->exch_pending) {
    rb_set_error("rb_learner_unit_activity: the gradients of the last learn call still wait for rb_learner_finish_grads, which reads the "
                 "activations this call overwrites");
    return RB_ERR_STATE;
  }
  if (l->dw_deferred) {
    rb_set_error("rb_learner_unit_activity: the last learn call left the hidden layer's weight gradient to the fused optimiser pass "
                 "(RB_LEARNER_FUSE_FC_H_DW), which reads the activations this call overwrites; call rb_learner_clip_adam first");
    return RB_ERR_STATE;
  }
  const Layout& L = l->L;
  const int B = L.B;
  ImgSrc src;
  memset(&src, 0, sizeof(src));
  src.u8_states = states_dev; src.B = B;
  const NetPtrs on = net_ptrs(L, l->p_online, l->zero_noise);        // eval mode (model.py:46), the online network's B rows only
  const int rc = forward(l, B, 0, src, on, on, stream);
  if (rc != RB_OK) return rc;
  RedoMap M;
  redo_map(L, 0.0f, &M);
  RB_LAUNCH(k_unit_activity, dim3((unsigned)M.n_units), dim3(RB_REDO_THREADS), stream, M, (const float*)l->act[0], (const float*)l->act[1],
            (const float*)l->act[2], (const float*)l->h, B, L.nconv, 2 * L.H, (int)accumulate, activity_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

int rb_learner_dormant_mask(rb_learner_t* l, const double* activity_dev, double tau, uint8_t* mask_dev, int32_t* counts_dev,
                            float* scores_dev, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_dormant_mask: NULL handle (l)");
  RB_REQUIRE(activity_dev != nullptr, "rb_learner_dormant_mask: NULL activity_dev");
  RB_REQUIRE(mask_dev != nullptr, "rb_learner_dormant_mask: NULL mask_dev");
  RB_REQUIRE(counts_dev != nullptr, "rb_learner_dormant_mask: NULL counts_dev");
  RB_REQUIRE(tau >= 0.0 && tau < (double)INFINITY, "rb_learner_dormant_mask: tau must be finite and >= 0, got %g", tau);   // (also NaN)
  RedoMap M;
  redo_map(l->L, 0.0f, &M);
  RB_LAUNCH(k_dormant_mask, dim3((unsigned)M.n_layers), dim3(RB_REDO_THREADS), stream, M, activity_dev, tau, mask_dev, counts_dev, scores_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

int rb_learner_recycle_units(rb_learner_t* l, const uint8_t* mask_dev, float noisy_std, uint64_t seed, uint64_t draw, int32_t with_target,
                             float* exp_avg_dev, float* exp_avg_sq_dev, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_recycle_units: NULL handle (l)");
  RB_REQUIRE(mask_dev != nullptr, "rb_learner_recycle_units: NULL mask_dev");
  RB_REQUIRE(noisy_std >= 0.0f && noisy_std < INFINITY, "rb_learner_recycle_units: noisy_std must be finite and >= 0, got %g", (double)noisy_std);
  RB_REQUIRE((exp_avg_dev == nullptr) == (exp_avg_sq_dev == nullptr), "rb_learner_recycle_units: pass both moment buffers or neither");
  RB_REQUIRE(((uintptr_t)exp_avg_dev | (uintptr_t)exp_avg_sq_dev) % 16 == 0, "rb_learner_recycle_units: the moment buffers must be 16-byte aligned");
  RB_REQUIRE(l->L.n_params * 4 < (int64_t)0x7fffffff, "rb_learner_recycle_units: the flat parameter buffer must be smaller than 2 GiB");
  RB_FLUSH_UPDATE(l, stream);          // a pending pass belongs to the OLD tensors: it runs before the recycle, never after it
  RedoMap M;
  redo_map(l->L, noisy_std, &M);
  for (int k = 0; k < M.n_layers; ++k)
    RB_REQUIRE(M.l[k].in_first < 0 || M.l[k].row / M.l[k].in_per <= RB_REDO_MAX_IN, "rb_learner_recycle_units: layer %d reads from more than %d units",
               k, RB_REDO_MAX_IN);
  RB_LAUNCH(k_recycle_units, dim3((unsigned)M.n_units), dim3(RB_REDO_THREADS), stream, M, mask_dev, l->p_online,
            with_target ? l->p_target : (float*)nullptr, exp_avg_dev, exp_avg_sq_dev, seed ^ RB_REDO_KEY_TAG, draw);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

}  // extern "C"
