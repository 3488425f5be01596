// noisy_rows.h — the NoisyLinear layers of the batched act path with ONE NOISE SAMPLE PER ROW (rb_learner_act_batch_rows): the S
// streams of a vectorised actor each explore with their own perturbation of the weights.  Included by learner.hip only.
//
// With per-row noise the weight W[m] = mu + sigma * (eps_out[m] eps_in[m]^T) differs for every row m, so the streamed kernels of
// nl_fwd.h (which form W once in registers and share it over the rows) cannot serve it; a loop over rows would read the 51 MB
// of the hidden layer's mu | sigma n times.  The factorised form reads them once:
//
//   y[m][j] = sum_k x[m][k] mu[j][k]  +  eo[m][j] * sum_k (x[m][k] ein[m][k]) sigma[j][k]  +  bmu[j] + bsigma[j] eo[m][j]
//
// — two contractions over the same streamed mu and sigma tiles, the second with the pre-scaled activations x (.) ein[m] as its row
// operand, eo[m][j] applied in the epilogue.  Same bytes as the shared-noise forward, twice the MFMAs, on a launch that waits on
// HBM.  This is NOT the reference's rounding order (model.py:39,44 forms W, then contracts): that order cannot be kept without
// giving up weight sharing.  Measured against the per-row oracle in f32: at most 0.27 of the act tolerance.
//
// k_nlr_fwd keeps k_nl_fwd3's structure (line-wide buffer loads of the weight tiles, a per-wave LDS transpose to the operand
// layout, waves splitting K and meeting once in LDS) and shares its per-wave setup (nl_fwd.h NlFwdWave); eps_in is never staged in LDS (n = 64 rows of K = 3136 would be 800 KB) —
// the scaled activations arrive k-blocked (rb_blocked_index) from the pass in front: k_block_copy_rows for the hidden layer, the
// hidden kernel's own epilogue for the output layer.  The accumulators and the cross-wave reduction buffer are twice fwd3's, so
// the M tile stops at MT = 2 (32 rows per workgroup: 32 KB of reduction buffer + 36 KB of transpose tiles, 24 float4 of
// activations in flight per lane); more rows are more m-chunks, as in the shared-noise path below 128 rows.
#pragma once
#include "nl_fwd.h"
#include "noise_body.h"

// ------------------------------------------------------------------ the generator --
// noise_rows[i][*] for i in [0, rows): the layout of rb_learner_noise_layout per row, floats no tensor covers written as zero.
// raw != NULL: f32 [rows][draws] N(0,1) in the reference's order (parity hook); else Philox + Box-Muller keyed WITHOUT device
// state: row r = row0 + i, draw pair j -> rb_philox(seed, ctr_hi = round, ctr_lo = (r << 32) | j), the same f(x) and the same
// two-normals-per-block use as rb_noise_body.  grid = (blocks over n_noise, rows).
__global__ __launch_bounds__(256) void k_noise_rows(float* noise_rows, const float* raw, NoiseMap map, int n_noise, uint64_t seed,
                                                     uint64_t round, int row0) {
  const int ri = (int)blockIdx.y;
  float* dst = noise_rows + (int64_t)ri * n_noise;
  const int draws = map.seg_begin[8];
  for (int p = (int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x; p < n_noise; p += (int)gridDim.x * (int)blockDim.x) {
    int i = -1;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int cnt = map.seg_begin[q + 1] - map.seg_begin[q];
      if (p >= map.dst[q] && p < map.dst[q] + cnt) i = map.seg_begin[q] + (p - map.dst[q]);
    }
    float f = 0.0f;
    if (i >= 0) {
      float x;
      if (raw) {
        x = raw[(int64_t)ri * draws + i];
      } else {
        const rb_philox_out r = rb_philox(seed, round, ((uint64_t)(uint32_t)(row0 + ri) << 32) | (uint64_t)(uint32_t)(i >> 1));
        const float u1 = ((float)(r.v[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float u2 = ((float)(r.v[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float rad = sqrtf(-2.0f * logf(u1));
        const float ang = 6.283185307179586f * u2;
        x = (i & 1) ? rad * sinf(ang) : rad * cosf(ang);
      }
      const float s = x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f);
      f = s * sqrtf(fabsf(x));
    }
    dst[p] = f;
  }
}

// ------------------------------------------------------------- scaled activations --
// k_block_copy with the two scaled copies next to it: row-major feat [rows][F] -> k-blocked feat_b over F columns, and k-blocked
// feat_s over 2F columns = feat (.) ein_hv[row] | feat (.) ein_ha[row]  (ein: noise row `row`, floats [ein_off, ein_off + 2F)).
__global__ __launch_bounds__(256) void k_block_copy_rows(const float* x, int rows, int F, const float* noise_rows, int n_noise,
                                                          int ein_off, float* xb, float* xs) {
  const int64_t total = (int64_t)rows * F;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / F), k = (int)(i % F);
    const float v = x[i];
    const float* e = noise_rows + (int64_t)row * n_noise + ein_off;
    xb[rb_blocked_index(row, k, rows)] = v;
    xs[rb_blocked_index(row, k, rows)] = v * e[k];
    xs[rb_blocked_index(row, F + k, rows)] = v * e[F + k];
  }
}

// ------------------------------------------------------------------ streamed layer --
struct NlRowsArgs {
  const float* x;           // k-blocked activations over M rows (rb_blocked_index)
  const float* xs;          // k-blocked SCALED activations x (.) ein[m] over M rows
  const float *mu, *sigma;  // [N][K]
  const float *bmu, *bsigma;
  const float* noise_rows;  // [M][n_noise]
  int n_noise, eout_off;    // eo[m][n] = noise_rows[m * n_noise + eout_off + n]
  int M, K;
  int n_groups;
  NlRowGroup grp[2];        // x_off: column offset into x, ein_off: column offset into xs; tile_begin counts 16-row tiles
  float* out;               // [M][ld_out]
  float* out_blocked;       // optional k-blocked copy over ld_out columns
  float* out_scaled;        // optional k-blocked copy of out (.) noise_rows[m][next_ein_off + n] (the next layer's xs)
  int next_ein_off;
  int ld_out;
  int relu;
};

// grid = (16-row weight tiles, 1, m-chunks of 16 MT rows), block = 512.  Preconditions as k_nl_fwd3 (plan_caps fast_fc).
template <int MT>
__global__ __launch_bounds__(64 * RB_NL_FWD_WAVES) void k_nlr_fwd(NlRowsArgs a) {
  __shared__ float s_red[RB_NL_FWD_WAVES][8 * MT][64];   // slots [0, 4 MT): the mu sums, [4 MT, 8 MT): the sigma sums
  __shared__ __attribute__((aligned(16))) float s_wt[RB_NL_FWD_WAVES][2][16 * RB_NL_FWD_WT_LD];
  const int lane = rb_lane(), wave = rb_wave();
  const int M = a.M;
  const int m0 = (int)blockIdx.z * (16 * MT);
  if (m0 >= M) return;                                   // block-uniform
  const int g = (a.n_groups > 1 && (int)blockIdx.x >= a.grp[1].tile_begin) ? 1 : 0;
  const NlRowGroup grp = a.grp[g];
  const int row0 = grp.row_begin + ((int)blockIdx.x - grp.tile_begin) * 16;
  const int row_end = grp.row_begin + grp.row_cnt;
  const int K = a.K;
  const NlFwdWave wv(K, row0, row_end);
  const int r = wv.r, q = wv.q, lr = wv.lr, lk = wv.lk;
  const rb_buf bmu = rb_make_buf(a.mu), bsg = rb_make_buf(a.sigma), bx = rb_make_buf(a.x), bxs = rb_make_buf(a.xs);
  float* wtm = &s_wt[wave][0][0];                         // [16 rows][RB_NL_FWD_WT_LD] of mu
  float* wts = &s_wt[wave][1][0];                         // ... of sigma
  unsigned xo[MT], xso[MT];
  wv.x_offsets<MT>(grp.x_off, M, 0, m0, M, xo);
  wv.x_offsets<MT>(grp.ein_off, M, 0, m0, M, xso);
  const unsigned xstep = (unsigned)M * 64u;               // bytes between consecutive 16-wide k chunks of the activations
  const float b_mu = a.bmu[wv.nb], b_sg = a.bsigma[wv.nb];

  rb_f32x4 accm[MT], accs[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e) { accm[mt][e] = 0.0f; accs[mt][e] = 0.0f; }

  constexpr int RING = MT >= 2 ? 3 : 4;
  float4 r_mu[RING][2], r_sg[RING][2], r_x[RING][2][MT], r_xs[RING][2][MT];
  auto load_w = [&](int d, int b) {
    const unsigned so = (unsigned)b * 128u;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      r_mu[d][i] = rb_ld4_buf(bmu, wv.wo[i], so);
      r_sg[d][i] = rb_ld4_buf(bsg, wv.wo[i], so);
    }
  };
  auto load_x = [&](int d, int b) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const unsigned so = (unsigned)(2 * b + h) * xstep;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        r_x[d][h][mt] = rb_ld4_buf(bx, xo[mt], so);
        r_xs[d][h][mt] = rb_ld4_buf(bxs, xso[mt], so);
      }
    }
  };
  auto stage = [&](int d) {                          // the transpose: what was loaded as 8 rows x 128 B becomes the operand layout
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<float4*>(&wtm[(8 * i + lr) * RB_NL_FWD_WT_LD + 4 * lk]) = r_mu[d][i];
      *reinterpret_cast<float4*>(&wts[(8 * i + lr) * RB_NL_FWD_WT_LD + 4 * lk]) = r_sg[d][i];
    }
  };
  auto mfmas = [&](int d) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 m4 = *reinterpret_cast<const float4*>(&wtm[r * RB_NL_FWD_WT_LD + 16 * h + 4 * q]);
      const float4 s4 = *reinterpret_cast<const float4*>(&wts[r * RB_NL_FWD_WT_LD + 16 * h + 4 * q]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) { accm[mt] = rb_mfma16(r_x[d][h][mt].x, m4.x, accm[mt]); accs[mt] = rb_mfma16(r_xs[d][h][mt].x, s4.x, accs[mt]); }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) { accm[mt] = rb_mfma16(r_x[d][h][mt].y, m4.y, accm[mt]); accs[mt] = rb_mfma16(r_xs[d][h][mt].y, s4.y, accs[mt]); }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) { accm[mt] = rb_mfma16(r_x[d][h][mt].z, m4.z, accm[mt]); accs[mt] = rb_mfma16(r_xs[d][h][mt].z, s4.z, accs[mt]); }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) { accm[mt] = rb_mfma16(r_x[d][h][mt].w, m4.w, accm[mt]); accs[mt] = rb_mfma16(r_xs[d][h][mt].w, s4.w, accs[mt]); }
    }
  };
  // k_nl_fwd3's EXACT ring, written out: no slot is ever loaded with a block past the wave's range.  (As one function template
  // shared with k_nl_fwd3 the same schedule cost k_nlr_fwd<1> two registers, 168 -> 170, and with them its third wave per SIMD.)
  const int nsc = wv.nsc, b0 = wv.b0;
#pragma unroll
  for (int d = 0; d < RING; ++d)
    if (d < nsc) { load_w(d, b0 + d); load_x(d, b0 + d); }   // wave-uniform
  const int full = nsc / RING * RING;
  const int steady = full >= RING ? full - RING : 0;      // the LAST full round refills only the slots the tail will consume
  for (int sc0 = 0; sc0 < steady; sc0 += RING) {
#pragma unroll
    for (int d = 0; d < RING; ++d) {
      const int sc = sc0 + d;
      stage(d);
      load_w(d, b0 + sc + RING);                           // refill the weight half of this ring slot (sc + RING < full <= nsc)
      rb_wave_sync();                                    // the tiles are private to the wave: LDS executes its ops in order
      mfmas(d);
      load_x(d, b0 + sc + RING);                           // ... and its activation half, once the MFMAs have read it
      rb_wave_sync();                                    // tile reads done before the next block overwrites them
      RB_SCHED_FENCE();
    }
  }
  if (steady < full) {                                   // wave-uniform: the last full round
#pragma unroll
    for (int d = 0; d < RING; ++d) {
      const int sc = steady + d;
      const bool refill = sc + RING < nsc;               // wave-uniform
      stage(d);
      if (refill) load_w(d, b0 + sc + RING);
      rb_wave_sync();
      mfmas(d);
      if (refill) load_x(d, b0 + sc + RING);
      rb_wave_sync();
      RB_SCHED_FENCE();
    }
  }
#pragma unroll
  for (int d = 0; d < RING; ++d) {                       // tail: the blocks the last refills brought in, no more loads
    if (full + d < nsc) {                                // wave-uniform
      stage(d);
      rb_wave_sync();
      mfmas(d);
      rb_wave_sync();
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s_red[wave][mt * 4 + e][lane] = accm[mt][e];
      s_red[wave][4 * MT + mt * 4 + e][lane] = accs[mt][e];
    }
  __syncthreads();
  for (int idx = (int)threadIdx.x; idx < 4 * MT * 64; idx += 64 * RB_NL_FWD_WAVES) {
    const int slot = idx >> 6, l = idx & 63;
    float vm = s_red[0][slot][l], vs = s_red[0][4 * MT + slot][l];
#pragma unroll
    for (int wv = 1; wv < RB_NL_FWD_WAVES; ++wv) { vm += s_red[wv][slot][l]; vs += s_red[wv][4 * MT + slot][l]; }
    const int mt = slot >> 2, e = slot & 3;
    const int m = m0 + 16 * mt + 4 * (l >> 4) + e;
    const int n = row0 + (l & 15);
    if (m < M && n < row_end) {
      const float* nz = a.noise_rows + (int64_t)m * a.n_noise;
      const float eo = nz[a.eout_off + n];
      float o = (vm + eo * vs) + (b_mu + b_sg * eo);      // (n == wv.nb for every cell that is stored)
      if (a.relu) o = fmaxf(o, 0.0f);
      a.out[(int64_t)m * a.ld_out + n] = o;
      if (a.out_blocked) a.out_blocked[rb_blocked_index(m, n, M)] = o;
      if (a.out_scaled) a.out_scaled[rb_blocked_index(m, n, M)] = o * nz[a.next_ein_off + n];
    }
  }
}

// -------------------------------------------------------------------- plain fallback --
// The same two-sum form for configurations the streamed kernels refuse (plan_caps fast_fc == 0, e.g. a hidden size that is no
// multiple of 32): one wave per output cell, row-major operands, eps_in read in place.  Not the hot path.
struct NlRowsGenericArgs {
  const float* x;           // [M][ldx]
  int ldx;
  const float *mu, *sigma, *bmu, *bsigma;   // [N][K], [N]
  const float* noise_rows;
  int n_noise, ein_off, eout_off;
  int M, N, K;
  int split_row;            // weight rows >= split_row read x at column x_off1 and eps_in at ein_off + ein_off1
  int x_off1, ein_off1;
  float* out;               // [M][ld_out]
  int ld_out, relu;
};
// grid = ceil(M * N / 4), block = 256 (4 waves, one output cell each)
__global__ __launch_bounds__(256) void k_nlr_generic(NlRowsGenericArgs a) {
  const int64_t cell = (int64_t)blockIdx.x * 4 + rb_wave();
  const int64_t cells = (int64_t)a.M * a.N;
  const bool live = cell < cells;                        // wave-uniform
  const int64_t cc = live ? cell : cells - 1;
  const int m = (int)(cc / a.N), n = (int)(cc % a.N);
  const bool second = n >= a.split_row;
  const float* x = a.x + (int64_t)m * a.ldx + (second ? a.x_off1 : 0);
  const float* nz = a.noise_rows + (int64_t)m * a.n_noise;
  const float* ein = nz + a.ein_off + (second ? a.ein_off1 : 0);
  const float* mu = a.mu + (int64_t)n * a.K;
  const float* sg = a.sigma + (int64_t)n * a.K;
  float sm = 0.0f, ss = 0.0f;
  for (int k = rb_lane(); k < a.K; k += 64) {
    const float xv = x[k];
    sm += xv * mu[k];
    ss += (xv * ein[k]) * sg[k];
  }
  sm = rb_wave_sum(sm);
  ss = rb_wave_sum(ss);
  if (live && rb_lane() == 0) {
    const float eo = nz[a.eout_off + n];
    float o = (sm + eo * ss) + (a.bmu[n] + a.bsigma[n] * eo);
    if (a.relu) o = fmaxf(o, 0.0f);
    a.out[(int64_t)m * a.ld_out + n] = o;
  }
}
