// feature_gram.h — the rank of the learned features (srank: Kumar, Agarwal, Ghosh, Levine, "Implicit Under-Parameterization
// Inhibits Data-Efficient Deep RL", ICLR 2021; feature rank: Lyle, Rowland, Dabney, "Understanding and Preventing Capacity Loss in
// RL", ICLR 2022): the capture of one batch's feature rows and the sample-side Gram matrix K = Phi Phi^T in double.  Included by
// learner.hip only, after unit_recycle.h (whose eval-mode forward sequence the capture repeats).  Never on the per-step path.
//
// The spectrum is taken on the host from K (rainbow_amd/feature_rank.py): a Gram matrix accumulated in f32 puts a noise floor of
// about sigma_max sqrt(d 2^-24) under the singular values, which swamps srank's 1 % threshold; in double the floor is
// sigma_max sqrt(d 2^-53).  k_gram_f64 therefore widens the f32 rows exactly and accumulates on v_mfma_f64_16x16x4_f64.
//
// Summation order.  Every element K[i][j] is ONE chain over k = 0, 4, 8, ... in ascending order, four k per MFMA, in one wave of one
// workgroup: the reduction is never split.  The order depends on d alone — not on n, on the grid, on ld, or on where (i, j) falls in
// its tile — so K is bit-repeatable, the K of the first m rows is the top-left block of the K of all rows, and K is symmetric bit for
// bit (an off-diagonal value is computed once and stored twice).
#pragma once
#include "learner_internal.h"

#define RB_GRAM_TILE 64           // rows of Phi per panel: a workgroup computes a 64 x 64 tile of K, wave w the 32 x 32 quadrant (w >> 1, w & 1)
#define RB_GRAM_KC 32             // k per staged chunk
#define RB_GRAM_ROW 36            // floats between panel rows in LDS: 32 + 4, so that the 16 rows x 4 k a wave reads per operand
                                  // (word row * 36 + k) fall on 64 different banks and every row stays 16-byte aligned
#define RB_GRAM_THREADS 256
#define RB_GRAM_MAX_N 4096

// this thread's two quads of the panel rows [row0, row0 + 64) x columns [k0, k0 + 32): zero beyond row n and beyond column d (the
// columns [d, ld) and the rows >= n may hold anything, NaN included: they never enter a sum).  A quad that starts below d ends at
// or below ld (both are multiples of 4), so the 16-byte load stays inside its row.
__device__ __forceinline__ void rb_gram_fetch(const float* phi, int row0, int k0, int n, int d, int ld, float4 v[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q = (int)threadIdx.x + u * RB_GRAM_THREADS;
    const int row = row0 + (q >> 3), k = k0 + (q & 7) * 4;
    float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (row < n && k < d) {
      x = rb_ld4(phi + row * ld + k);
      if (k + 1 >= d) x.y = 0.0f;
      if (k + 2 >= d) x.z = 0.0f;
      if (k + 3 >= d) x.w = 0.0f;
    }
    v[u] = x;
  }
}
__device__ __forceinline__ void rb_gram_put(float* panel, const float4 v[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q = (int)threadIdx.x + u * RB_GRAM_THREADS;
    rb_st4(panel + (q >> 3) * RB_GRAM_ROW + (q & 7) * 4, v[u]);
  }
}

extern "C" {

// One workgroup per tile pair (ti <= tj) of the upper triangle, numbered column by column: (0,0), (0,1), (1,1), (0,2), ...
// The two row panels are staged through LDS as f32 in chunks of 32 k (the next chunk's 16-byte loads are in flight under the MFMAs of
// this one) and widened at the register.  A diagonal tile stages one panel and skips the quadrant below the diagonal.
// 4 n ld < 2^31 and n <= 4096 (host-checked): every index fits 32 bits.
__global__ __launch_bounds__(RB_GRAM_THREADS) void k_gram_f64(const float* phi, int n, int d, int ld, double* gram) {
  __shared__ float s_a[RB_GRAM_TILE * RB_GRAM_ROW];
  __shared__ float s_b[RB_GRAM_TILE * RB_GRAM_ROW];
  int ti = (int)blockIdx.x, tj = 0;
  while (ti > tj) { ti -= tj + 1; ++tj; }                            // block-uniform
  const bool diag = ti == tj;
  const int lane = rb_lane(), wave = rb_wave();
  const int wr = wave >> 1, wc = wave & 1;
  const bool work = !(diag && wr > wc);                               // wave-uniform
  const float* s_bp = diag ? s_a : s_b;
  rb_f64x4 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[m][c][r] = 0.0;
  float4 va[2], vb[2];
  rb_gram_fetch(phi, ti * RB_GRAM_TILE, 0, n, d, ld, va);
  if (!diag) rb_gram_fetch(phi, tj * RB_GRAM_TILE, 0, n, d, ld, vb);
  const int a_word = (wr * 32 + (lane & 15)) * RB_GRAM_ROW + (lane >> 4);
  const int b_word = (wc * 32 + (lane & 15)) * RB_GRAM_ROW + (lane >> 4);
  for (int k0 = 0; k0 < d; k0 += RB_GRAM_KC) {
    rb_gram_put(s_a, va);
    if (!diag) rb_gram_put(s_b, vb);
    __syncthreads();
    if (k0 + RB_GRAM_KC < d) {
      rb_gram_fetch(phi, ti * RB_GRAM_TILE, k0 + RB_GRAM_KC, n, d, ld, va);
      if (!diag) rb_gram_fetch(phi, tj * RB_GRAM_TILE, k0 + RB_GRAM_KC, n, d, ld, vb);
    }
    if (work) {
#pragma unroll
      for (int kk = 0; kk < RB_GRAM_KC; kk += 4) {
        const double a0 = (double)s_a[a_word + kk], a1 = (double)s_a[a_word + 16 * RB_GRAM_ROW + kk];
        const double b0 = (double)s_bp[b_word + kk], b1 = (double)s_bp[b_word + 16 * RB_GRAM_ROW + kk];
        acc[0][0] = rb_mfma16_f64(a0, b0, acc[0][0]);
        acc[0][1] = rb_mfma16_f64(a0, b1, acc[0][1]);
        acc[1][0] = rb_mfma16_f64(a1, b0, acc[1][0]);
        acc[1][1] = rb_mfma16_f64(a1, b1, acc[1][1]);
      }
    }
    __syncthreads();
  }
  if (!work) return;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int li = wr * 32 + m * 16 + rb_mfma16_f64_row(r, lane), lj = wc * 32 + c * 16 + (lane & 15);
        const int i = ti * RB_GRAM_TILE + li, j = tj * RB_GRAM_TILE + lj;
        if (i >= n || j >= n || (diag && li > lj)) continue;
        const double v = acc[m][c][r];
        gram[i * n + j] = v;
        if (i != j) gram[j * n + i] = v;
      }
}

int rb_gram_f64(const float* phi_dev, int32_t n, int32_t d, int32_t ld, double* gram_dev, rb_stream_t stream) {
  RB_REQUIRE(phi_dev != nullptr, "rb_gram_f64: NULL phi_dev");
  RB_REQUIRE(gram_dev != nullptr, "rb_gram_f64: NULL gram_dev");
  RB_REQUIRE(n >= 1 && n <= RB_GRAM_MAX_N, "rb_gram_f64: n must be in [1, %d], got %d", RB_GRAM_MAX_N, (int)n);
  RB_REQUIRE(d >= 1, "rb_gram_f64: d must be >= 1, got %d", (int)d);
  RB_REQUIRE(ld >= d, "rb_gram_f64: ld must be >= d = %d, got %d", (int)d, (int)ld);
  RB_REQUIRE(ld % 4 == 0, "rb_gram_f64: ld must be a multiple of 4, got %d", (int)ld);
  RB_REQUIRE((uintptr_t)phi_dev % 16 == 0, "rb_gram_f64: phi_dev must be 16-byte aligned");
  RB_REQUIRE((uintptr_t)gram_dev % 8 == 0, "rb_gram_f64: gram_dev must be 8-byte aligned");
  RB_REQUIRE((int64_t)4 * n * ld < ((int64_t)1 << 31), "rb_gram_f64: n * ld floats must stay below 2 GiB, got n = %d, ld = %d", (int)n, (int)ld);
  const int T = (int)rb_div_up(n, RB_GRAM_TILE);
  RB_LAUNCH(k_gram_f64, dim3((unsigned)(T * (T + 1) / 2)), dim3(RB_GRAM_THREADS), (hipStream_t)stream, phi_dev, (int)n, (int)d, (int)ld, gram_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

int rb_learner_feature_dim(const rb_learner_config_t* cfg, int32_t which, int32_t* d) {
  Layout L;
  const int rc = make_layout(cfg, &L);
  if (rc != RB_OK) return rc;
  RB_REQUIRE(d != nullptr, "rb_learner_feature_dim: d is NULL");
  RB_REQUIRE(which == RB_FEATURES_HIDDEN || which == RB_FEATURES_CONV, "rb_learner_feature_dim: unknown selector (which) %d", (int)which);
  *d = which == RB_FEATURES_HIDDEN ? 2 * L.H : L.F;
  return RB_OK;
}

int rb_learner_features(rb_learner_t* l, const uint8_t* states_dev, int32_t which, float* out_dev, int32_t ld, rb_stream_t stream_) {
  RB_REQUIRE(l != nullptr, "rb_learner_features: NULL handle (l)");
  RB_REQUIRE(states_dev != nullptr, "rb_learner_features: NULL states_dev");
  RB_REQUIRE(out_dev != nullptr, "rb_learner_features: NULL out_dev");
  RB_REQUIRE(which == RB_FEATURES_HIDDEN || which == RB_FEATURES_CONV, "rb_learner_features: unknown selector (which) %d", (int)which);
  const Layout& L = l->L;
  const int B = L.B, d = which == RB_FEATURES_HIDDEN ? 2 * L.H : L.F;
  RB_REQUIRE(ld >= d, "rb_learner_features: ld must be >= the feature dimension %d, got %d", d, (int)ld);
  hipStream_t stream = (hipStream_t)stream_;
  RB_FLUSH_UPDATE(l, stream);
  if (l->exch_pending) {
    rb_set_error("rb_learner_features: the gradients of the last learn call still wait for rb_learner_finish_grads, which reads the "
                 "activations this call overwrites");
    return RB_ERR_STATE;
  }
  if (l->dw_deferred) {
    rb_set_error("rb_learner_features: the last learn call left the hidden layer's weight gradient to the fused optimiser pass "
                 "(RB_LEARNER_FUSE_FC_H_DW), which reads the activations this call overwrites; call rb_learner_clip_adam first");
    return RB_ERR_STATE;
  }
  ImgSrc src;
  memset(&src, 0, sizeof(src));
  src.u8_states = states_dev; src.B = B;
  const NetPtrs on = net_ptrs(L, l->p_online, l->zero_noise);        // eval mode, the online network's B rows (rb_learner_unit_activity)
  const int rc = forward(l, B, 0, src, on, on, stream);
  if (rc != RB_OK) return rc;
  // rows [0, B) of h [NI][2H], or of the last conv layer's activations [NI][cout][P] = [NI][F]: what rb_learner_debug_read hands out
  const float* rows = which == RB_FEATURES_HIDDEN ? l->h : l->act[L.nconv - 1];
  if (ld == d) {
    RB_HIP_TRY(hipMemcpyAsync(out_dev, rows, (size_t)B * d * 4, hipMemcpyDeviceToDevice, stream));
  } else {
#if defined(RB_HOST_INTERP)
    for (int b = 0; b < B; ++b)
      RB_HIP_TRY(hipMemcpyAsync(out_dev + (size_t)b * ld, rows + (size_t)b * d, (size_t)d * 4, hipMemcpyDeviceToDevice, stream));
#else
    RB_HIP_TRY(hipMemcpy2DAsync(out_dev, (size_t)ld * 4, rows, (size_t)d * 4, (size_t)d * 4, (size_t)B, hipMemcpyDeviceToDevice, stream));
#endif
  }
  return RB_OK;
}

}  // extern "C"
