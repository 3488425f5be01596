// adam_kernels.h — the optimiser pass as launches of its own (adam_body.h has the element bodies and the hosted form).
// Included by learner.hip only (non-template kernels, and rb_launch_adam_pending, which is defined here).
#pragma once
#include "learner_internal.h"
#include "nl_dw.h"

// (ClipAdamArgs, rb_adam_elem / rb_adam_quad and the hosted form of the pass: adam_body.h)
// Tile part of the fused optimiser pass (batch <= 32).  The hidden layer's weight gradient is a rank-B product,
// g_mu = dY^T X  (dY [B][2H], X [B][F], both L2-resident: 0.5 MB), g_sigma = g_mu * (eps_out x eps_in).  Writing it in the
// backward and reading it back here costs 2 x 25.7 MB of HBM traffic per step; instead a wave recomputes its 16 x 64
// tile with 32 MFMAs (nl_dw.h's tile setup and MFMA block, the ones the backward's norm-only pass ran: the same bits)
// while its p / m / v loads are in flight, and applies clip + Adam to mu and sigma right there: 6 array passes
// over the 6.4 M weights instead of 9.
struct FusedDwAdamArgs {
  NlDwArgs dw;                 // operands of the weight gradient (g_* unused)
  int64_t mu_off, sigma_off;   // offsets of the [2H][F] mu / sigma arrays inside p, m, v (and g)
  int dw_x, n_tile_blocks;     // 256-column block columns; 256-thread tile blocks = dw_x * (2H / 16)
  int write_grads;             // tests: also store the (unclipped... as clip_grad_norm_ leaves it: clipped) gradient tile
};
// Each tile is taken by TWO workgroup slots: slot 0 updates mu, slot 1 sigma (both recompute the same 32 MFMAs — 0.4 GFLOP
// extra per step against 24 fewer live registers per lane: 4 waves per SIMD instead of 2, no spills; the single-slot
// version measured 36.5 us per launch against 35.0 for the plain streaming pass, i.e. slower despite 13 % fewer bytes).
template <bool WT>
__device__ __forceinline__ void rb_fused_dw_adam_tile(const ClipAdamArgs& a, const FusedDwAdamArgs& f, int b2, float coef) {
  const NlDwArgs& d = f.dw;
  const int which = b2 & 1, b = b2 >> 1;                 // 0: mu, 1: sigma
  const NlDwTile t = rb_nl_dw_tile(d, b % f.dw_x, b / f.dw_x, 256);
  if (!t.live) return;                                    // wave-uniform (no norm slot to zero here)
  const int col4 = t.col4(t.kt);
  const bool cv = t.col_ok(t.kt);
  const int64_t arr = which ? f.sigma_off : f.mu_off;
  // operands of the gradient tile first (they gate the MFMAs), then the 12 parameter / moment quads (they gate the update)
  float avs[8];
  float4 xs[8];
#pragma unroll
  for (int st = 0; st < 8; ++st) {                        // this tile zeroes the quad it loaded
    const int m = 4 * st + t.q;
    const bool mv = m < d.M;
    avs[st] = t.dy_masked(d.dy, d.ldy, m, d.M);
    xs[st] = rb_ld4(d.x + (int64_t)(mv ? m : d.M - 1) * d.ldx + t.pr.x_off + col4);
    if (!mv) { xs[st].x = 0.0f; xs[st].y = 0.0f; xs[st].z = 0.0f; xs[st].w = 0.0f; }
  }
  const float4 e4 = rb_ld4(d.ein + t.pr.ein_off + col4);
  float eo4[4];
  int64_t off[4];
  float4 P[4], M[4], V[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int n = t.row_clamped(e);                       // clamped rows are loaded (legal) and never stored
    eo4[e] = d.eout[n];
    off[e] = arr + (int64_t)n * d.K + col4;
    P[e] = rb_ld4(a.p + off[e]); M[e] = rb_ld4(a.m + off[e]); V[e] = rb_ld4(a.v + off[e]);
  }
  rb_f32x4 acc[4], accb;                                  // (no bias sum here: accb stays unused)
  rb_nl_dw_zero(acc, accb);
  rb_nl_dw_mfma32(0, d.M, [&](int st) { return avs[st]; }, [&](int st) { return xs[st]; }, false, acc, accb);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (t.row(e) < t.row_end && cv) {
      float4 gr;
      gr.x = acc[0][e]; gr.y = acc[1][e]; gr.z = acc[2][e]; gr.w = acc[3][e];
      if (which) gr = rb_noisy_grad4(gr, eo4[e], e4);     // block-uniform: g_sigma = g_mu * (eps_out * eps_in), model.py:39,44
      rb_adam_quad(P[e], gr, M[e], V[e], coef, a);
      if (WT) {
        const unsigned o = (unsigned)(4 * off[e]);
        rb_st4_wt(a.p, o, P[e]); rb_st4_wt(a.m, o, M[e]); rb_st4_wt(a.v, o, V[e]);
      } else {
        rb_st4(a.p + off[e], P[e]); rb_st4(a.m + off[e], M[e]); rb_st4(a.v + off[e], V[e]);
      }
      if (f.write_grads) rb_st4(a.g + off[e], gr);         // as clip_grad_norm_ leaves .grad: scaled when the clip bites
    }
  }
}
#define RB_ADAM_MINWAVES 1
// EMA (never with FUSED: the tile pass's register budget shaped its design; k_target_ema follows that launch instead): the
// target's quads are loaded with the others and written behind them (adam_body.h rb_ema_elem).  An instantiation of its own,
// chosen by the host: with a.t == NULL the plain one runs, the kernel it has always been.
template <int RB_ADAM_UNROLL, bool WT, bool FUSED, bool EMA = false>   // float4 quadruples (p, g, m, v) in flight per thread; WT: write-through stores
__global__ __launch_bounds__(256, RB_ADAM_MINWAVES) void k_clip_adam(ClipAdamArgs a, FusedDwAdamArgs f) {
  static_assert(!(EMA && FUSED), "k_clip_adam: the fused tile pass has no in-pass EMA");
  __shared__ float s_red[18];      // [0, 16) rb_block_sum's wave slots; [16], [17] the bias-correction scalars (slots of their own:
                                   // thread 0 writes them while other waves may still be reading the wave slots of the sum —
                                   // the host interpreter's schedule turned that into a wrong clip coefficient for every thread
                                   // but thread 0 whenever the clip bit and the step number came from the device counter)
  const bool tile_block = FUSED && (int)blockIdx.x < f.n_tile_blocks;
  const int64_t n4 = (a.n >> 2) - (FUSED ? a.skip_len4 : 0);
  const int eb = FUSED ? (int)blockIdx.x - f.n_tile_blocks : (int)blockIdx.x;
  const int64_t base = (int64_t)eb * (256 * RB_ADAM_UNROLL) + threadIdx.x;
  float4 P[RB_ADAM_UNROLL], G[RB_ADAM_UNROLL], M[RB_ADAM_UNROLL], V[RB_ADAM_UNROLL];
  int64_t idx[RB_ADAM_UNROLL];
  if (!tile_block) {
#pragma unroll
    for (int u = 0; u < RB_ADAM_UNROLL; ++u) {
      int64_t i = base + u * 256;
      if (i >= n4) i = n4 > 0 ? n4 - 1 : 0;          // clamped load (always legal), masked store
      if (FUSED && i >= a.skip_lo4) i += a.skip_len4;
      idx[u] = i;
      P[u] = rb_ld4(a.p + 4 * i); G[u] = rb_ld4(a.g + 4 * i); M[u] = rb_ld4(a.m + 4 * i); V[u] = rb_ld4(a.v + 4 * i);
    }
  }
  const bool ema_copy = EMA && a.tau == 1.0f;                       // uniform
  float4 TG[EMA ? RB_ADAM_UNROLL : 1];
  if (EMA && !ema_copy) {
#pragma unroll
    for (int u = 0; u < RB_ADAM_UNROLL; ++u) TG[u] = rb_ld4(a.t + 4 * idx[u]);
  }
  if (a.batch_status && *a.batch_status != 0) {                     // block-uniform (every block reads the same word)
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.norm_out) *a.norm_out = 0.0f;
    return;
  }
  float acc = 0.0f;
  for (int i = (int)threadIdx.x; i < a.nparts; i += 256) acc += a.part[i];
  acc = rb_block_sum(acc, s_red);
  const float total = sqrtf(acc);
  float coef = a.max_norm / (total + 1e-6f);
  if (coef > 1.0f) coef = 1.0f;                                    // clamp(max=1.0)
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.norm_out) *a.norm_out = total;
  if (a.step_dev) {                                                // block-uniform
    if (threadIdx.x == 0) {
      const double t = (double)*a.step_dev;
      const double bc1 = 1.0 - pow(a.beta1, t), bc2 = 1.0 - pow(a.beta2, t);
      s_red[16] = (float)(-(a.lr / bc1));
      s_red[17] = (float)sqrt(bc2);
    }
    __syncthreads();
    a.neg_step_size = s_red[16];
    a.bc2_sqrt = s_red[17];
  }
  if (tile_block) {
    rb_fused_dw_adam_tile<WT>(a, f, (int)blockIdx.x, coef);
    return;
  }
#pragma unroll
  for (int u = 0; u < RB_ADAM_UNROLL; ++u) {
    if (base + u * 256 >= n4) continue;
    const int64_t i = idx[u];
    rb_adam_quad(P[u], G[u], M[u], V[u], coef, a);
    if (WT) {
      const unsigned off = (unsigned)(16 * i);
      rb_st4_wt(a.p, off, P[u]); rb_st4_wt(a.m, off, M[u]); rb_st4_wt(a.v, off, V[u]);
    } else {
      rb_st4(a.p + 4 * i, P[u]); rb_st4(a.m + 4 * i, M[u]); rb_st4(a.v + 4 * i, V[u]);
    }
    if (coef < 1.0f) rb_st4(a.g + 4 * i, G[u]);
    if (EMA) {
      rb_ema_quad(TG[u], P[u], a.tau, ema_copy);
      if (WT) rb_st4_wt(a.t, (unsigned)(16 * i), TG[u]);
      else rb_st4(a.t + 4 * i, TG[u]);
    }
  }
  // tail (n % 4 elements): last block's first threads
  if (blockIdx.x == gridDim.x - 1) {
    const int64_t t = ((a.n >> 2) << 2) + threadIdx.x;
    if (t < a.n) {
      float p = a.p[t], g = a.g[t], m = a.m[t], v = a.v[t];
      rb_adam_elem(p, g, m, v, coef, a);
      a.p[t] = p; a.m[t] = m; a.v[t] = v;
      if (coef < 1.0f) a.g[t] = g;
      if (EMA) {
        float tg = p;
        if (!ema_copy) { tg = a.t[t]; rb_ema_elem(tg, p, a.tau); }
        a.t[t] = tg;
      }
    }
  }
}

extern "C" {      // (C linkage: the names a kernel trace has always shown for these two)

// g_sigma = g_mu * (eps_out[n] * eps_in[k]) for the hidden layer, from the noise snapshot of the learn call that produced g_mu:
// what RB_LEARNER_IMPLICIT_SIGMA's backward left out, for every consumer of the flat gradient other than the hosted pass
__global__ __launch_bounds__(256) void k_materialize_sigma(float* g, int64_t mu4, int64_t len4, int f4, int split_row,
                                                            const float* eout, const float* ein, const int32_t* clipped) {
  if (*clipped != 0) return;          // the optimiser pass has stored the scaled gradients already (block-uniform)
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < len4; j += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(j / f4), cq = (int)(j - (int64_t)row * f4);
    const float eo = eout[row];
    const float4 e = rb_ld4(ein + 4 * (int64_t)(cq + (row >= split_row ? f4 : 0)));
    rb_st4(g + 4 * (mu4 + len4 + j), rb_noisy_grad4(rb_ld4(g + 4 * (mu4 + j)), eo, e));
  }
}

__global__ void k_store_adam_args(ClipAdamArgs a, ClipAdamArgs* dst) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *dst = a;
}

// the pending optimiser pass (adam_body.h) as a launch of its own: flush_update (optimizer_host.h), and what the replay's
// sample_impl falls back to when the sampler variant that can host the pass does not fit the replay's window length
__global__ __launch_bounds__(256) void k_adam_pending(const ClipAdamArgs* ad) {
  __shared__ float s_adam[18];
  rb_adam_hosted_block<4>(ad, (int)blockIdx.x, (int)gridDim.x, s_adam);
}

// the same with the target EMA (arguments with a target pointer: rb_launch_adam_pending is told)
__global__ __launch_bounds__(256) void k_adam_pending_ema(const ClipAdamArgs* ad) {
  __shared__ float s_adam[18];
  rb_adam_hosted_block<4, true>(ad, (int)blockIdx.x, (int)gridDim.x, s_adam);
}

// The EMA as a launch of its own: t <- t + tau (p - t) over n floats (t = p for tau == 1), skipped like the optimiser pass when
// the batch status says the draw failed (status may be NULL).  Behind the fused tile pass (k_clip_adam<4, true, true>, which
// carries no EMA), and rb_learner_target_ema.  Grid-stride over quads, the n % 4 tail by block 0's first threads.
__global__ __launch_bounds__(256) void k_target_ema(float* t, const float* p, int64_t n, float tau, const int32_t* status) {
  if (status && *status != 0) return;                               // block-uniform
  const bool copy = tau == 1.0f;
  const int64_t n4 = n >> 2;
  for (int64_t i0 = (int64_t)blockIdx.x * 1024 + threadIdx.x; i0 < n4; i0 += (int64_t)gridDim.x * 1024) {
    float4 P[4], T[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = i0 + u * 256 < n4 ? i0 + u * 256 : n4 - 1;  // clamped load, masked store
      P[u] = rb_ld4(p + 4 * i);
      if (!copy) T[u] = rb_ld4(t + 4 * i);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = i0 + u * 256;
      if (i >= n4) continue;
      rb_ema_quad(T[u], P[u], tau, copy);
      rb_st4(t + 4 * i, T[u]);
    }
  }
  if (blockIdx.x == 0) {
    const int64_t e = (n4 << 2) + threadIdx.x;
    if (e < n) {
      float tg = p[e];
      if (!copy) { tg = t[e]; rb_ema_elem(tg, p[e], tau); }
      t[e] = tg;
    }
  }
}

}  // extern "C"

// (declared in adam_body.h: replay.hip calls it across translation units)
int rb_launch_adam_pending(const ClipAdamArgs* args_dev, int blocks, void* stream, bool ema) {
  if (ema) RB_LAUNCH_T("clip_adam:k_adam_pending", k_adam_pending_ema, dim3((unsigned)blocks), dim3(256), (hipStream_t)stream, args_dev);
  else RB_LAUNCH_T("clip_adam:k_adam_pending", k_adam_pending, dim3((unsigned)blocks), dim3(256), (hipStream_t)stream, args_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}
