// act_fc.h — the noisy-linear layers of the act path (Agent.act / evaluate_q on ONE un-batched state): one weight row per wave,
// lanes sweep K in float4s (K % 4 == 0), so a layer is one coalesced sweep of its mu | sigma instead of the training kernels'
// 16-row tiles (nl_fwd.h: 2-3 workgroups for one image).  Same arithmetic as model.py:42-46 (f32, fused multiply-add
// accumulation in a fixed order).  rb_act_fc_prefetch requests a row's weights ahead of the activations they will meet.
// Device functions only, called by act_path.h k_act_fused, which includes this; needs nl_common.h (NlWeights, rb_noisy4) and
// rb_device.h (coherent buffer loads, write-through stores, the wave sum).
#pragma once
#include "nl_common.h"
#include "rb_device.h"

struct ActFcArgs {
  const float* x;      // [K] per row group (x_off1 for rows >= split_row)
  NlWeights w;
  int K, n_rows;
  int split_row;       // first row of the second stream (fc_h: advantage stream, fc_z: advantage atoms)
  int x_off1, ein_off1;
  float* out;          // [n_rows]
  int relu;
  int mu_only;         // eval mode (model.py:46): W = mu, b = b_mu — sigma / eps are not even read
};

// One weight row of a noisy layer; the 64 lanes of one wave call (row < n_rows, wave-uniform).  PQ > 0: the row's mu | sigma
// quads are already in `pm` / `ps` (rb_act_fc_prefetch, requested before the previous phase's wait); the activations and eps_in
// are loaded here (coherent).
template <int PQ>
__device__ __forceinline__ void rb_act_fc_row(const ActFcArgs& a, int row, const float4* pm, const float4* ps) {
  const int lane = rb_lane();
  const bool g1 = row >= a.split_row;
  const float* mu = a.w.mu + (int64_t)row * a.K;
  const float* sg = a.w.sigma + (int64_t)row * a.K;
  const rb_buf bx = rb_make_buf(a.x + (g1 ? a.x_off1 : 0));
  const float* ein = a.w.ein + (g1 ? a.ein_off1 : 0);
  const float eo = a.mu_only ? 0.0f : a.w.eout[row];
  const int n4 = a.K >> 2;
  float acc = 0.0f;
  // Chunks of 4 quads per lane (4 float4 of every operand in flight), in the same order for every PQ: the prefetched form gives
  // the bits of PQ = 0.  PQ > 0: the chunk count is a compile-time number (the host picked PQ with K / 4 <= 64 PQ), so that the
  // prefetched quads are indexed by constants and stay in registers
  auto chunk = [&](int b0, const float4* cm, const float4* cs, int have) {
    float4 m[4], s[4], xv[4], e[4];
    float live[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int i = b0 + u * 64 + lane;
      live[u] = i < n4 ? 1.0f : 0.0f;
      if (i > n4 - 1) i = n4 - 1;
      xv[u] = rb_ld4_buf_sc1(bx, 16u * (unsigned)i, 0u);
      if (u < have) { m[u] = cm[u]; s[u] = cs[u]; }
      else { m[u] = rb_ld4(mu + 4 * i); s[u] = a.mu_only ? m[u] : rb_ld4(sg + 4 * i); }
      e[u] = a.mu_only ? m[u] : rb_ld4(ein + 4 * i);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float4 w4 = a.mu_only ? m[u] : rb_noisy4(m[u], s[u], eo, e[u]);
      float part = 0.0f;
      part = fmaf(w4.x, xv[u].x, part);
      part = fmaf(w4.y, xv[u].y, part);
      part = fmaf(w4.z, xv[u].z, part);
      part = fmaf(w4.w, xv[u].w, part);
      acc = fmaf(live[u], part, acc);
    }
  };
  if constexpr (PQ > 0) {
#pragma unroll
    for (int ch = 0; ch < (PQ + 3) / 4; ++ch)
      if (ch * 256 < n4) chunk(ch * 256, pm + 4 * ch, ps + 4 * ch, PQ - 4 * ch < 4 ? PQ - 4 * ch : 4);
  } else {
    for (int b0 = 0; b0 < n4; b0 += 4 * 64) chunk(b0, nullptr, nullptr, 0);
  }
  acc = rb_wave_sum(acc);
  if (lane == 0) {
    float o = acc + (a.mu_only ? a.w.bmu[row] : (a.w.bmu[row] + a.w.bsigma[row] * eo));   // model.py:44,46
    if (a.relu) o = fmaxf(o, 0.0f);
    rb_st1_wt(a.out, 4u * (unsigned)row, o);
  }
}
template <int PQ>
__device__ __forceinline__ void rb_act_fc_prefetch(const ActFcArgs& a, int row, float4* pm, float4* ps) {
  const int lane = rb_lane();
  const int n4 = a.K >> 2;
  if (row >= a.n_rows) row = a.n_rows - 1;                       // (a wave without a row still issues legal loads)
#pragma unroll
  for (int j = 0; j < PQ; ++j) {
    int i = j * 64 + lane;                                       // chunk j / 4, u = j % 4: index b0 + u * 64 + lane
    if (i > n4 - 1) i = n4 - 1;
    pm[j] = rb_ld4(a.w.mu + (int64_t)row * a.K + 4 * i);
    ps[j] = a.mu_only ? pm[j] : rb_ld4(a.w.sigma + (int64_t)row * a.K + 4 * i);
  }
}
