// nl_dw.h — the NoisyLinear weight gradient:
// g_mu[n][k] = sum_m dy[m][n] * x[m][x_off + k] ; g_sigma = g_mu * (eps_out[n]*eps_in[k]) ;
// g_bmu[n] = sum_m dy[m][n] ; g_bsigma = g_bmu * eps_out[n].   One writer per element.
// A wave owns a 16-row x 64-column tile.  The pieces of a tile — its setup, the 32-sample MFMA block, the epilogue, the commit
// of the wave's sum of squares — are written once here; the four bodies below and the optimiser pass's recomputed tile
// (adam_kernels.h rb_fused_dw_adam_tile) are load schedules around them, so the bits of a tile cannot differ between them.
#pragma once
#include "nl_common.h"

struct NlDwProblem {
  int row_begin, row_cnt;    // weight rows == columns of dy
  int x_off, ein_off;
  int tile_begin;            // first 16-row tile index in grid.y
};
struct NlDwArgs {
  const float* dy;           // [M][ldy]
  const float* x;            // [M][ldx]
  int ldy, ldx, M, K;
  int n_prob;
  NlDwProblem prob[2];
  float *g_mu, *g_sigma, *g_bmu, *g_bsigma;
  const float *eout, *ein;
  float* sq_part;            // optional: one slot per (block, wave) receiving the sum of squares of what that wave wrote
                             // (feeds clip_grad_norm_ without another pass over the 27 MB gradient)
  int ct;                    // > 0: pipelined body, `ct` column tiles per wave (M <= 32; 4: every tile's operands in flight before
                             // the first MFMA, rb_nl_dw_body_pipe_all); 0: one tile per wave
  int no_sigma;              // 1: g_sigma is formed for the sum of squares only and NOT stored (the hosted optimiser pass forms it
                             // again from g_mu and the same noise, adam_body.h)
  int norm_only;             // 1: the weight-gradient tiles are computed for their sum of squares only and NOT stored (the
                             // optimiser pass recomputes each tile while it streams the parameters, k_clip_adam<FUSED>);
                             // the bias gradients are still written
  // Replica exchange: the reduction rows are the all-gathered factor blocks of `world` ranks — row m lives in
  // block m / rpb at row m % rpb, blocks `bstride` floats apart (rpb == 0: one plain matrix) — and the result is the
  // replica MEAN: scale = 1 / world (a power of two for 2/4/8 replicas, i.e. exact; 1.0f otherwise leaves every bit alone)
  int rpb;
  int64_t bstride;
  float scale;
  // ... and every rank's gradient is noisy with ITS OWN epsilon (each replica resamples its own noise, agent.py:49,74):
  // g_sigma = mean_r g_mu_r * (eps_out_r x eps_in_r).  The gathered blocks therefore carry each rank's noise buffer:
  // rank r's eps_out / eps_in of this layer sit at noise_blocks + r * bstride + eout_noff / ein_noff.
  const float* noise_blocks;
  int64_t eout_noff, ein_noff;
};

// ------------------------------------------------------------------------- tile pieces --
// The tile of this wave in a grid of (column blocks, 16-row tiles): wave w owns columns [cols_per_block * bx + 64 w, +64) — and,
// in the pipelined bodies, the tiles 256 columns further on.  Lane (c, q) holds dY column / weight row row0 + c as the A operand
// of reduction slot q, the activation quad at column kt + 4 c as B, and the accumulator rows row0 + 4 q + e.
struct NlDwTile {
  NlDwProblem pr;
  int K;
  int kt;                    // first column of the wave's (first) tile
  bool live;                 // the wave has columns (wave-uniform); when it has none only K, kt, live and av_ok are set
  int row0, row_end;
  int c, q;
  int arow;                  // this lane's dY column, clamped into the problem
  bool av_ok;                // ... and whether it was in range
  __device__ __forceinline__ int row(int e) const { return row0 + 4 * q + e; }
  __device__ __forceinline__ int row_clamped(int e) const { const int n = row(e); return n < row_end ? n : row_end - 1; }
  __device__ __forceinline__ bool col_ok(int kt_) const { return kt_ + 4 * c < K; }
  __device__ __forceinline__ int col4(int kt_) const { const int col = kt_ + 4 * c; return col < K ? col : K - 4; }   // clamped: always a legal address
  // eps_out of the four accumulator rows (requested with the first operand loads: asked for after the loop it costs a second round trip)
  __device__ __forceinline__ void load_eout(const float* eout, float (&eo4)[4]) const {
#pragma unroll
    for (int e = 0; e < 4; ++e) eo4[e] = eout[row_clamped(e)];
  }
  // the dY operand of sample m of M, zero where the sample or this lane's row is out of range
  __device__ __forceinline__ float dy_masked(const float* dy, int ldy, int m, int M) const {
    const bool mv = m < M;
    return (mv && av_ok) ? dy[(int64_t)(mv ? m : M - 1) * ldy + arow] : 0.0f;
  }
};
__device__ __forceinline__ NlDwTile rb_nl_dw_tile(const NlDwArgs& a, int bx, int by, int cols_per_block) {
  NlDwTile t;
  const int lane = rb_lane();
  t.K = a.K;
  t.kt = bx * cols_per_block + rb_wave() * 64;
  t.live = t.kt < a.K;
  t.av_ok = false;                                       // (set before the early return: the struct is copied, and a bool must hold a value)
  if (!t.live) return t;
  t.pr = a.prob[(a.n_prob > 1 && by >= a.prob[1].tile_begin) ? 1 : 0];
  t.row0 = t.pr.row_begin + (by - t.pr.tile_begin) * 16;
  t.row_end = t.pr.row_begin + t.pr.row_cnt;
  t.c = lane & 15; t.q = lane >> 4;
  t.arow = t.row0 + t.c;
  t.av_ok = t.arow < t.row_end;
  if (!t.av_ok) t.arow = t.row_end - 1;
  return t;
}
// ... for a body that owns a norm slot: a wave without columns zeroes its slot and is told to leave (wave-uniform: the bodies
// have no barriers)
__device__ __forceinline__ bool rb_nl_dw_tile_or_leave(const NlDwArgs& a, int bx, int by, int cols_per_block, int slot_base, NlDwTile& t) {
  t = rb_nl_dw_tile(a, bx, by, cols_per_block);
  if (!t.live && a.sq_part && rb_lane() == 0) a.sq_part[slot_base + rb_wave()] = 0.0f;
  return t.live;
}

// One 32-sample block of a tile: the 8 reduction steps of 4 samples from sample mb of M (uniform).  av(st) and x(st) hand over
// step st's operands MASKED — zero where the sample or the lane's row is out of range — and are asked right before the step's
// MFMAs, so a body that masks late waits for one step's loads at a time (with all eight masked up front the compiler waited
// for the whole block before the first MFMA).  How a body masks (select, multiply by 0 / 1, zero the loaded quad) stays with
// the body: each keeps the form it was measured with, and nothing here depends on which.
template <class Av, class X>
__device__ __forceinline__ void rb_nl_dw_mfma32(int mb, int M, Av av, X x, bool do_bias, rb_f32x4 (&acc)[4], rb_f32x4& accb) {
  // (named copies: updated in place through the reference, the compiler keeps acc[4] as one 16-float value and shuffles it
  // between the accumulation and the vector registers around every step)
  rb_f32x4 a0 = acc[0], a1 = acc[1], a2 = acc[2], a3 = acc[3], ab = accb;
#pragma unroll
  for (int st = 0; st < 8; ++st) {
    if (mb + 4 * st < M) {                                 // uniform
      const float a = av(st);
      const float4 b = x(st);
      a0 = rb_mfma16(a, b.x, a0);
      a1 = rb_mfma16(a, b.y, a1);
      a2 = rb_mfma16(a, b.z, a2);
      a3 = rb_mfma16(a, b.w, a3);
      if (do_bias) ab = rb_mfma16(a, 1.0f, ab);              // wave-uniform
    }
  }
  acc[0] = a0; acc[1] = a1; acc[2] = a2; acc[3] = a3; accb = ab;
}
__device__ __forceinline__ void rb_nl_dw_zero(rb_f32x4 (&acc)[4], rb_f32x4& accb) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { accb[e] = 0.0f; acc[0][e] = 0.0f; acc[1][e] = 0.0f; acc[2][e] = 0.0f; acc[3][e] = 0.0f; }
}

// The store-and-square half of an epilogue: one row's quad of g_mu and g_sigma, and the bias pair.
__device__ __forceinline__ void rb_nl_dw_store_sq(const NlDwArgs& a, int n, int col4, const float4& gm, const float4& gs,
                                                  bool store, bool store_sigma, float& sq) {
  if (store) {                                             // wave-uniform
    rb_st4(a.g_mu + (int64_t)n * a.K + col4, gm);          // (write-through stores measured no gain here)
    if (store_sigma) rb_st4(a.g_sigma + (int64_t)n * a.K + col4, gs);
  }
  sq = fmaf(gm.x, gm.x, sq); sq = fmaf(gm.y, gm.y, sq); sq = fmaf(gm.z, gm.z, sq); sq = fmaf(gm.w, gm.w, sq);
  sq = fmaf(gs.x, gs.x, sq); sq = fmaf(gs.y, gs.y, sq); sq = fmaf(gs.z, gs.z, sq); sq = fmaf(gs.w, gs.w, sq);
}
__device__ __forceinline__ void rb_nl_dw_bias_sq(const NlDwArgs& a, int n, float gb, float gbs, float& sq) {
  a.g_bmu[n] = gb;
  a.g_bsigma[n] = gbs;
  sq = fmaf(gb, gb, sq); sq = fmaf(gbs, gbs, sq);
}
// The epilogue of the tile at column kt: g_mu = acc, g_sigma = g_mu * (eps_out * eps_in), stored unless norm_only / no_sigma say
// otherwise (wave-uniform), their squares into sq, and the bias pair by the first column tile.  (rb_nl_dw_body stored without
// looking at the two flags before it shared this epilogue; the plan sets them only with a pipelined body or the tiled GEMM —
// defer_dw needs p.pipe, implicit_sigma needs p.pipe or the GEMM — so it never sees them set: the same behaviour for every
// reachable plan.)
__device__ __forceinline__ void rb_nl_dw_epilogue(const NlDwArgs& a, const NlDwTile& t, int kt, const rb_f32x4 (&acc)[4],
                                                  const rb_f32x4& accb, const float4& e4, const float (&eo4)[4], float& sq) {
  const bool cv = t.col_ok(kt), do_bias = kt == 0;
  const int col4 = t.col4(kt);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int n = t.row(e);
    if (n < t.row_end) {
      const float eo = eo4[e];
      if (cv) {
        float4 gm;
        gm.x = acc[0][e]; gm.y = acc[1][e]; gm.z = acc[2][e]; gm.w = acc[3][e];
        rb_nl_dw_store_sq(a, n, col4, gm, rb_noisy_grad4(gm, eo, e4), !a.norm_only, !a.no_sigma, sq);
      }
      if (do_bias && t.c == 0) rb_nl_dw_bias_sq(a, n, accb[e], accb[e] * eo, sq);
    }
  }
}
// The wave's sum of squares into its norm slot (wave-uniform; also the tiled GEMM's bodies, fc_gemm.h)
__device__ __forceinline__ void rb_nl_sq_commit(float* sq_part, int slot_base, float sq) {
  if (sq_part) {
    const int lane = rb_lane(), wave = rb_wave();
    sq = rb_wave_sum(sq);
    if (lane == 0) sq_part[slot_base + wave] = sq;
  }
}

// ------------------------------------------------------------------------------ bodies --
// One tile per wave, any M.  grid = (256-column tiles, 16-row tiles), block = 256.
__device__ __forceinline__ void rb_nl_dw_body(const NlDwArgs& a, int bx, int by, int slot_base) {
  NlDwTile t;
  if (!rb_nl_dw_tile_or_leave(a, bx, by, 256, slot_base, t)) return;
  const int q = t.q, col4 = t.col4(t.kt);
  rb_f32x4 acc[4], accb;
  rb_nl_dw_zero(acc, accb);
  const float4 e4 = rb_ld4(a.ein + t.pr.ein_off + col4);
  float eo4[4];
  t.load_eout(a.eout, eo4);
  // 8 reduction steps (32 samples) of loads per trip, and the NEXT trip's loads requested before this trip's MFMAs: at batch 256 the
  // eight trips were eight dependent round trips (13.3 of the output layer's 14.4 us backward launch, round6_wg_timeline_b256.txt).
  // Same MFMAs in the same order: bit-identical.
  auto issue = [&](int mb, float (&avs)[8], float4 (&xs)[8]) {
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      const int m = mb + 4 * st + q;
      const int mcl = m < a.M ? m : a.M - 1;
      avs[st] = a.dy[(int64_t)mcl * a.ldy + t.arow];
      xs[st] = rb_ld4(a.x + (int64_t)mcl * a.ldx + t.pr.x_off + col4);
    }
  };
  auto mfmas = [&](int mb, const float (&avs)[8], const float4 (&xs)[8]) {   // this body masks by select, after the loads
    rb_nl_dw_mfma32(mb, a.M,
                    [&](int st) { return (mb + 4 * st + q < a.M && t.av_ok) ? avs[st] : 0.0f; },
                    [&](int st) {
                      const bool mv = mb + 4 * st + q < a.M;
                      float4 x;
                      x.x = mv ? xs[st].x : 0.0f; x.y = mv ? xs[st].y : 0.0f; x.z = mv ? xs[st].z : 0.0f; x.w = mv ? xs[st].w : 0.0f;
                      return x;
                    },
                    t.kt == 0, acc, accb);
  };
  {
    float avs0[8], avs1[8];
    float4 xs0[8], xs1[8];
    issue(0, avs0, xs0);
    for (int mb = 0; mb < a.M; mb += 64) {
      const bool second = mb + 32 < a.M;                   // uniform
      if (second) issue(mb + 32, avs1, xs1);
      mfmas(mb, avs0, xs0);
      if (second) {
        if (mb + 64 < a.M) issue(mb + 64, avs0, xs0);
        mfmas(mb + 32, avs1, xs1);
      }
    }
  }
  float sq = 0.0f;
  rb_nl_dw_epilogue(a, t, t.kt, acc, accb, e4, eo4, sq);
  rb_nl_sq_commit(a.sq_part, slot_base, sq);
}

// Replica-exchange variant (rb_learner_finish_grads): the reduction rows are `M / rpb` rank blocks of rpb rows each.  Every
// rank's block is reduced on its own (same MFMA order as the single-device bodies, so acc_r has the bits that rank alone
// would have produced), then folded in rank order:  g_mu += acc_r ;  g_sigma += acc_r * (eps_out_r * eps_in_r) ; the sums
// are scaled by 1 / world at the end — the arithmetic of "every replica computes its gradient, then all-reduce(mean)".
// A wave owns 64 columns: 256 per 4-wave block, 512 per 8-wave block.
__device__ __forceinline__ void rb_nl_dw_body_ranks(const NlDwArgs& a, int bx, int by, int slot_base) {
  NlDwTile t;
  if (!rb_nl_dw_tile_or_leave(a, bx, by, (int)blockDim.x, slot_base, t)) return;
  const int col4 = t.col4(t.kt);
  const bool cv = t.col_ok(t.kt), do_bias = t.kt == 0;
  const int nranks = a.M / a.rpb;
  rb_f32x4 gm[4], gs[4], gbm, gbs;
  rb_nl_dw_zero(gm, gbm);
  rb_nl_dw_zero(gs, gbs);
  for (int r = 0; r < nranks; ++r) {
    const float* dy = a.dy + (int64_t)r * a.bstride;
    const float* x = a.x + (int64_t)r * a.bstride;
    const float* nz = a.noise_blocks + (int64_t)r * a.bstride;
    const float4 e4 = rb_ld4(nz + a.ein_noff + t.pr.ein_off + col4);
    float eo4[4];
    t.load_eout(nz + a.eout_noff, eo4);
    rb_f32x4 acc[4], accb;
    rb_nl_dw_zero(acc, accb);
    for (int mb = 0; mb < a.rpb; mb += 32) {
      float avs[8];
      float4 xs[8];
#pragma unroll
      for (int st = 0; st < 8; ++st) {                       // this body zeroes the quad it loaded
        const int m = mb + 4 * st + t.q;
        const bool mv = m < a.rpb;
        avs[st] = t.dy_masked(dy, a.ldy, m, a.rpb);
        xs[st] = rb_ld4(x + (int64_t)(mv ? m : a.rpb - 1) * a.ldx + t.pr.x_off + col4);
        if (!mv) { xs[st].x = 0.0f; xs[st].y = 0.0f; xs[st].z = 0.0f; xs[st].w = 0.0f; }
      }
      rb_nl_dw_mfma32(mb, a.rpb, [&](int st) { return avs[st]; }, [&](int st) { return xs[st]; }, do_bias, acc, accb);
    }
    const float ej[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        gm[j][e] = gm[j][e] + acc[j][e];
        gs[j][e] = gs[j][e] + acc[j][e] * (eo4[e] * ej[j]);
      }
      gbm[e] = gbm[e] + accb[e];
      gbs[e] = gbs[e] + accb[e] * eo4[e];
    }
  }
  float sq = 0.0f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int n = t.row(e);
    if (n < t.row_end) {
      if (cv) {
        float4 m4, s4;
        m4.x = gm[0][e] * a.scale; m4.y = gm[1][e] * a.scale; m4.z = gm[2][e] * a.scale; m4.w = gm[3][e] * a.scale;
        s4.x = gs[0][e] * a.scale; s4.y = gs[1][e] * a.scale; s4.z = gs[2][e] * a.scale; s4.w = gs[3][e] * a.scale;
        rb_nl_dw_store_sq(a, n, col4, m4, s4, true, true, sq);
      }
      if (do_bias && t.c == 0) rb_nl_dw_bias_sq(a, n, gbm[e] * a.scale, gbs[e] * a.scale, sq);
    }
  }
  rb_nl_sq_commit(a.sq_part, slot_base, sq);
}

// Pipelined bodies for M <= 32 (one reduction pass per tile): a wave walks `ct` column tiles 256 apart with the same dY operand.
// grid.x = ceil(K / (256 ct)); the sum-of-squares slot of a wave covers all its tiles.  What the two share: the dY operand, the
// activation row pointers, and the 0 / 1 factor these bodies mask the activations with.
struct NlDwPipe {
  NlDwTile t;
  float eo4[4], avs[8], xmask[8];
  const float* xrow[8];
  __device__ __forceinline__ void begin(const NlDwArgs& a) {       // (t is set: rb_nl_dw_tile_or_leave)
    t.load_eout(a.eout, eo4);
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      const int m = 4 * st + t.q;
      const bool mv = m < a.M;
      avs[st] = t.dy_masked(a.dy, a.ldy, m, a.M);
      xrow[st] = a.x + (int64_t)(mv ? m : a.M - 1) * a.ldx + t.pr.x_off;
      xmask[st] = mv ? 1.0f : 0.0f;
    }
  }
  __device__ __forceinline__ int kt(int j) const { return t.kt + j * 256; }
  // the operands of column tile j (clamped: always a legal address)
  __device__ __forceinline__ void load(const NlDwArgs& a, int j, float4& e4, float4 (&xs)[8]) const {
    const int col4 = t.col4(kt(j));
    e4 = rb_ld4(a.ein + t.pr.ein_off + col4);
#pragma unroll
    for (int st = 0; st < 8; ++st) xs[st] = rb_ld4(xrow[st] + col4);
  }
  // ... and its 40 MFMAs and epilogue
  __device__ __forceinline__ void tile(const NlDwArgs& a, int j, const float4& e4, const float4 (&xs)[8], float& sq) const {
    rb_f32x4 acc[4], accb;
    rb_nl_dw_zero(acc, accb);
    rb_nl_dw_mfma32(0, a.M, [&](int st) { return avs[st]; },
                    [&](int st) {                          // these bodies mask by the 0 / 1 factor
                      float4 x;
                      x.x = xs[st].x * xmask[st]; x.y = xs[st].y * xmask[st]; x.z = xs[st].z * xmask[st]; x.w = xs[st].w * xmask[st];
                      return x;
                    },
                    kt(j) == 0, acc, accb);
    rb_nl_dw_epilogue(a, t, kt(j), acc, accb, e4, eo4, sq);
  }
};
// One tile ahead: tile j+1's activations are requested before tile j is multiplied and stored — with one tile per wave every
// wave of the launch loaded, then multiplied, then stored at the same time (a read burst followed by a write burst).
__device__ __forceinline__ void rb_nl_dw_body_pipe(const NlDwArgs& a, int bx, int by, int slot_base) {
  NlDwPipe p;
  const int ct = a.ct;
  if (!rb_nl_dw_tile_or_leave(a, bx, by, ct * 256, slot_base, p.t)) return;
  p.begin(a);
  float4 xs[8], xn[8], e4, e4n;
  p.load(a, 0, e4, xs);
  float sq = 0.0f;
  for (int j = 0; j < ct; ++j) {
    if (p.kt(j) >= a.K) break;                           // wave-uniform
    p.load(a, j + 1 < ct ? j + 1 : j, e4n, xn);
    p.tile(a, j, e4, xs, sq);
    e4 = e4n;
#pragma unroll
    for (int st = 0; st < 8; ++st) xs[st] = xn[st];
  }
  rb_nl_sq_commit(a.sq_part, slot_base, sq);
}
// All tiles ahead (ct == 4): the operands of ALL CT column tiles of a wave are requested before the first MFMA.  The one-tile-ahead
// form turns a tile every ~3.3 us (13.2 us for the hidden layer's four: a round trip beside the launch's 39 MB is longer than a
// tile's 40 MFMAs), this one pays the trip once.  Same tiles, same order inside a tile: bit-identical gradients and norm partials.
template <int CT>
__device__ __forceinline__ void rb_nl_dw_body_pipe_all(const NlDwArgs& a, int bx, int by, int slot_base) {
  NlDwPipe p;
  if (!rb_nl_dw_tile_or_leave(a, bx, by, CT * 256, slot_base, p.t)) return;
  p.begin(a);
  float4 xa[CT][8], ea[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) p.load(a, j, ea[j], xa[j]);
  float sq = 0.0f;
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    if (p.kt(j) >= a.K) break;                           // wave-uniform
    p.tile(a, j, ea[j], xa[j], sq);
  }
  rb_nl_sq_commit(a.sq_part, slot_base, sq);
}
