// grad_finish.h — the small passes that finish activations and gradients: split reductions, the replica exchange's packing and
// finishing launches, the global-norm clip.  Included by learner.hip only (non-template kernels).
#pragma once
#include "learner_internal.h"
#include "nl_dw.h"

// ----------------------------------------------------------- small fused passes --
// h[img][n] = relu(sum_s part[s][img][n] + (bias_mu + bias_sigma*eps_out)[n])        model.py:44,72-73
__global__ __launch_bounds__(256) void k_fc_h_finish(const float* part, int splits, int NI, int H2, int n_online,
                                                      NetPtrs on, NetPtrs tg, float* h, float* h_blocked) {
  const int64_t total = (int64_t)NI * H2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int img = (int)(i / H2), n = (int)(i % H2);
    const NetPtrs& p = img < n_online ? on : tg;
    float acc = 0.0f;
    for (int s = 0; s < splits; ++s) acc += part[(int64_t)s * total + i];
    const float bias = p.h_bmu[n] + p.h_bsigma[n] * p.h_eout[n];
    const float o = fmaxf(acc + bias, 0.0f);
    h[i] = o;
    if (h_blocked) h_blocked[((int64_t)(n >> 4) * NI + img) * 16 + (n & 15)] = o;
  }
}

// row-major [rows][K] -> k-blocked copy (only when the generic conv path feeds the streamed FC kernels)
__global__ __launch_bounds__(256) void k_block_copy(const float* x, int rows, int K, float* xb) {
  const int64_t total = (int64_t)rows * K;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / K), k = (int)(i % K);
    xb[((int64_t)(k >> 4) * rows + row) * 16 + (k & 15)] = x[i];
  }
}

// dfeat[b][k] = (feat[b][k] > 0) * sum_s part[s][b][k]
__global__ __launch_bounds__(256) void k_dfeat_finish(const float* part, int splits, int64_t total, const float* feat,
                                                       float* dfeat) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const float fv = feat[i];
    float acc = 0.0f;
    for (int s0 = 0; s0 < splits; s0 += 8) {             // 8 partial loads in flight (a runtime-length loop of load-then-add
      float v[8];                                        // made every split its own dependent round trip)
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(s0 + u < splits ? s0 + u : splits - 1) * total + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += (s0 + u < splits) ? v[u] : 0.0f;
    }
    dfeat[i] = fv > 0.0f ? acc : 0.0f;
  }
}

// all conv layers' split slices in ONE launch (saves two dependent ~5 us launches per step)
struct ReduceLayer {
  const float* part;
  float *gw, *gb;
  int slices, cout, K;
  int64_t begin;          // first flat output index of this layer in the fused index space
};
struct ReduceAllArgs {
  ReduceLayer layer[3];
  int n_layers;
  int64_t total;
  float* sq_part;         // optional: one slot per block = sum of squares of the gradients this block produced
  // replica exchange: every reduced element is ALSO stored at copy_base + (its offset inside the flat gradient), i.e. into
  // the conv segment of this rank's exchange block
  const float* grads_base;
  float* copy_base;
  // tenant blocks behind the reduction's own: copy snap_n floats (the learn call's online noise, for the optimiser pass that
  // forms the hidden layer's sigma gradient itself: the launch hosting that pass resamples the noise)
  const float* snap_src;
  float* snap_dst;
  int snap_n;
  int32_t* snap_clear;      // ... and clear this word (ClipAdamArgs::pair_clipped: no scaled gradient has been stored for this step yet)
};
template <int N>
__device__ __forceinline__ float rb_sum_slices(const float* part, int64_t per, int64_t j, int slices) {
  float v[N];
#pragma unroll
  for (int u = 0; u < N; ++u) v[u] = part[(int64_t)(u < slices ? u : slices - 1) * per + j];   // clamped: always legal
  float acc = 0.0f;
#pragma unroll
  for (int u = 0; u < N; ++u) acc += (u < slices) ? v[u] : 0.0f;
  return acc;
}
__global__ __launch_bounds__(64) void k_reduce_conv_dw_all(ReduceAllArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ((a.total + 63) / 64) * 64) {                  // block-uniform: a snapshot tenant
    const int64_t j = i - ((a.total + 63) / 64) * 64;
    if (j < a.snap_n) a.snap_dst[j] = a.snap_src[j];
    if (j == 0 && a.snap_clear) *a.snap_clear = 0;
    return;
  }
  float my = 0.0f;
  if (i < a.total) {
  int li = 0;
  if (a.n_layers > 1 && i >= a.layer[1].begin) li = 1;
  if (a.n_layers > 2 && i >= a.layer[2].begin) li = 2;
  const ReduceLayer L = a.layer[li];
  const int64_t j = i - L.begin;
  const int64_t per = (int64_t)L.cout * (L.K + 1);
  // fixed add order (slice 0, 1, 2, ...), ALL slice loads of an element in flight at once: one memory round trip instead of
  // one per group of 32 (the first layer's 96 slices were three dependent trips: 4.5 of the kernel's 6 us).  Slice counts:
  // 96 / 64 / 64 at batch 32 (B images x row chunks), the same at larger batches (image groups).
  float acc = 0.0f;
  if (L.slices <= 32) acc = rb_sum_slices<32>(L.part, per, j, L.slices);           // (a layer's elements share the branch)
  else if (L.slices <= 64) acc = rb_sum_slices<64>(L.part, per, j, L.slices);
  else if (L.slices <= 96) acc = rb_sum_slices<96>(L.part, per, j, L.slices);
  else if (L.slices <= 128) acc = rb_sum_slices<128>(L.part, per, j, L.slices);    // data-efficient first layer: 4 chunks x 32
  else {                                                                            // (same left-to-right order, a trip per 32)
    for (int s0 = 0; s0 < L.slices; ++s0) acc += L.part[(int64_t)s0 * per + j];
  }
  const int co = (int)(j / (L.K + 1)), col = (int)(j % (L.K + 1));
  float* dst = col < L.K ? L.gw + (int64_t)co * L.K + col : L.gb + co;
  *dst = acc;
  if (a.copy_base) a.copy_base[dst - a.grads_base] = acc;
  my = acc * acc;
  }
  if (a.sq_part) {
    my = rb_wave_sum(my);
    if (threadIdx.x == 0) a.sq_part[blockIdx.x] = my;
  }
}

// the four factor matrices of the FC weight gradients, rows [0, B), packed into one block for the replica all-gather
struct PackArgs {
  const float* src[5];
  int64_t count[5];
  int64_t dst_off[5];
  float* dst;
};
__global__ __launch_bounds__(256) void k_pack_factors(PackArgs a) {
  const int which = (int)blockIdx.y;
  const int64_t n4 = a.count[which] >> 2;      // all segment sizes are multiples of 4 floats (fast_fc preconditions)
  const float* src = a.src[which];
  float* dst = a.dst + a.dst_off[which];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
    rb_st4(dst + 4 * i, rb_ld4(src + 4 * i));
  if (blockIdx.x == 0)
    for (int64_t i = (n4 << 2) + threadIdx.x; i < a.count[which]; i += blockDim.x) dst[i] = src[i];
}

// -------------------------------------------------------------- global-norm clip --
// clip_grad_norm_ (agent.py:97).  Stage 1: per-block sum of squares (fixed tree order).
__global__ __launch_bounds__(256) void k_sumsq(const float* g, int64_t n, float* part) {
  __shared__ float s_red[16];
  float acc = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    acc = fmaf(g[i], g[i], acc);
  acc = rb_block_sum(acc, s_red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
// rb_learner_finish_grads as ONE launch (three dependent-free jobs would otherwise queue as three ~10 us kernels on the
// replica step's critical path): k_finish_grads_tiled below
struct FinishArgs {
  NlDwArgs z, h;
  int z_x, z_n;                // grid.x and block count of the output layer's weight-gradient problem
  // conv range: g[i] = (sum over ranks, in rank order, of blocks[r * bstride + i]) * scale; part[b] = this block's sum of squares
  float* g; int64_t n; float* part; int nparts;
  const float* blocks; int64_t bstride; int world; float scale;
};
// The hidden layer's weight gradient on 128 x 128 LDS tiles (fc_gemm.h rb_fc_gemm_dw_ranks; 512-thread workgroups), the output
// layer's on 16-row tiles of 512 columns (nl_dw.h rb_nl_dw_body_ranks, all eight waves): block ranges [fc_h tiles, each with its
// slice of the conv range | fc_z tiles]
__global__ __launch_bounds__(RB_TG_THREADS) void k_finish_grads_tiled(FinishArgs a, int h_nt, int h_kt) {
  __shared__ __attribute__((aligned(16))) float lds[RB_TG_LDS];
  __shared__ float s_red[16];
  int b = (int)blockIdx.x;
  const int h_n = h_nt * h_kt;
  if (b < h_n) {
    // the conv range rides in the tile workgroups (a.nparts == h_n: one slice and one partial per workgroup): its per-element chain —
    // `world` loads, one add each — as 20 workgroups of their own was the launch's pole (22 of 40 us with the tile loop ablated:
    // every thread walked 8 elements x 8 ranks one dependent load at a time).  Here: one element per thread and trip, all ranks'
    // loads in flight, in front of the tile loop.
    float acc = 0.0f;
    for (int64_t i = (int64_t)b * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)a.nparts * blockDim.x) {
      float v = 0.0f;
      for (int r0 = 0; r0 < a.world; r0 += 8) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = a.blocks[(int64_t)(r0 + u < a.world ? r0 + u : a.world - 1) * a.bstride + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += (r0 + u < a.world) ? t[u] : 0.0f;      // rank order
      }
      v *= a.scale;
      a.g[i] = v;
      acc = fmaf(v, v, acc);
    }
    acc = rb_block_sum(acc, s_red);
    if (threadIdx.x == 0) a.part[b] = acc;
    rb_fc_gemm_dw_ranks(a.h, b / h_kt, b % h_kt, 8 * b, lds);
    return;
  }
  b -= h_n;
  if (b < a.z_n) rb_nl_dw_body_ranks(a.z, b % a.z_x, b / a.z_x, 8 * b);      // (all eight waves: 512 columns per workgroup)
}
// Stage 2: every block re-reduces the partials (same order everywhere), then scales its slice.
__global__ __launch_bounds__(256) void k_clip_scale(float* g, int64_t n, const float* part, int nparts, float max_norm,
                                                     float* norm_out) {
  __shared__ float s_red[16];
  float acc = 0.0f;
  for (int i = (int)threadIdx.x; i < nparts; i += (int)blockDim.x) acc += part[i];
  acc = rb_block_sum(acc, s_red);
  const float total = sqrtf(acc);
  float coef = max_norm / (total + 1e-6f);
  if (coef > 1.0f) coef = 1.0f;                                    // clamp(max=1.0)
  if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = total;
  if (coef < 1.0f)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
      g[i] *= coef;
}
