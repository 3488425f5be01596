// nl_fwd.h — the streamed NoisyLinear forward: out[m][n] = b[n] + sum_k x[m][x_off + k] * W[n][k]   (ReLU optional).
// One workgroup owns a 16-row weight tile for the whole K; its 8 waves take contiguous K ranges, stream mu | sigma through a ring
// of register slots, and meet once in LDS.  The per-wave setup is shared with the per-row-noise forward (noisy_rows.h
// k_nlr_fwd), which runs the EXACT form of the same ring schedule over its own loads, stage and MFMA steps.  (The schedule as
// one function template over those steps was tried: it cost k_nlr_fwd<1> two registers and its third wave per SIMD,
// profiles/nl_split_isa.txt; each kernel keeps its rounds written out.)
#pragma once
#include "nl_common.h"

struct NlRowGroup {
  int row_begin, row_cnt;   // weight rows of this stream
  int x_off, ein_off;       // column offset into x, offset into ein
  int tile_begin;           // first 16-row tile index of this group in grid.x
};
#define RB_NL_FWD_WAVES 8
struct NlFwdArgs {
  const float* x;           // k-blocked activations (rb_blocked_index)
  int m_base[2], m_cnt[2];
  NlWeights w[2];
  int K;
  int n_groups;
  NlRowGroup grp[2];        // tile_begin counts 16-row tiles here
  float* out;               // [rows_total][ld_out]
  float* out_blocked;       // optional k-blocked copy over ld_out columns
  int ld_out, rows_total;
  int relu;
};
#define RB_NL_FWD_MROWS 32
#define RB_NL_FWD_KMAX 4096          // eps_in slice staged in LDS (host checks K <= this)
#define RB_NL_FWD_WT_LD 36           // row stride (floats) of a wave's 16 x 32 weight tile: 16-byte reads of 16 rows hit 64 distinct banks

// ---------------------------------------------------------------------- per-wave setup --
// A wave's K range is a whole number of 32-wide blocks, balanced over the 8 waves (12/13 for the hidden layer); every load is a
// buffer load whose per-lane byte offset is fixed here, before the loop — the running block offset is wave-uniform and lives in
// an SGPR, one instruction per load (an earlier form built `pointer + 64-bit index` per load: ~50 instructions per block, as
// many issue cycles as the block's 16 MFMAs).
struct NlFwdWave {
  int nsc, b0, b_last;      // this wave's 32-wide blocks: how many, the first, the last (a wave without work: the layer's last)
  int r, q;                 // operand layout: weight row / activation row r of k-slot q
  int lr, lk;               // line-wide weight loads: 8 rows x 128 B per instruction
  int wrow[2];              // the two weight rows this lane loads (clamped into the group)
  unsigned wo[2];           // ... and their byte offsets
  int nb;                   // bias column: every epilogue cell of a thread is column row0 + (lane & 15), clamped
  __device__ __forceinline__ NlFwdWave(int K, int row0, int row_end) {
    const int lane = rb_lane(), wave = rb_wave();
    const int nblk = K / 32;                               // host guarantees K % 32 == 0
    const int base_n = nblk / RB_NL_FWD_WAVES, extra = nblk % RB_NL_FWD_WAVES;
    nsc = rb_wave_uniform(base_n + (wave < extra ? 1 : 0));
    b0 = rb_wave_uniform(wave * base_n + (wave < extra ? wave : extra));
    b_last = nsc > 0 ? b0 + nsc - 1 : nblk - 1;            // (a wave without work still issues the ring's loads: keep them in range)
    r = lane & 15; q = lane >> 4;
    lr = lane >> 3; lk = lane & 7;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int row = row0 + 8 * i + lr;
      if (row > row_end - 1) row = row_end - 1;
      wrow[i] = row;
      wo[i] = (unsigned)(((int64_t)row * K + 4 * lk) * 4);
    }
    nb = row0 + (lane & 15) < row_end ? row0 + (lane & 15) : row_end - 1;
  }
  __device__ __forceinline__ int blk_of(int sc) const { const int b = b0 + sc; return b < b_last ? b : b_last; }   // wave-uniform, clamped
  // byte offsets of this lane's float4 in the k-blocked activations over `rows` rows, column offset col_off, for the MT 16-row
  // m tiles from m0 (rows past M clamped); consecutive 16-wide k chunks are rows * 64 bytes apart
  template <int MT>
  __device__ __forceinline__ void x_offsets(int col_off, int rows, int m_base, int m0, int M, unsigned (&xo)[MT]) const {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      int m = m0 + 16 * mt + r;
      if (m > M - 1) m = M - 1;
      xo[mt] = (unsigned)((((int64_t)(col_off >> 4) * rows + m_base + m) * 16 + 4 * q) * 4);
    }
  }
};

// ------------------------------------------------------------------------------ kernel --
// No split-K partials: the 8 waves meet once in a 2 KB-per-wave LDS reduction; bias (+ReLU) is applied there and the result is
// written directly (row-major and, optionally, k-blocked for the next layer) — no partial-sum round trip, no separate finish
// kernel.  (A K-split across workgroups with a finish pass lost to this form twice, and ablation shows the activation re-reads
// through the 64 B/clk L1 cost as much as the weight stream itself: profiles/HISTORY.md.)
// grid = (16-row tiles, 1, 2 * m-chunks of 16 MT rows), block = 512
template <int MT>
__global__ __launch_bounds__(64 * RB_NL_FWD_WAVES) void k_nl_fwd3(NlFwdArgs a) {
  __shared__ float s_red[RB_NL_FWD_WAVES][4 * MT][64];
  __shared__ __attribute__((aligned(16))) float s_ein[RB_NL_FWD_KMAX];
  __shared__ __attribute__((aligned(16))) float s_wt[RB_NL_FWD_WAVES][16 * RB_NL_FWD_WT_LD];
  const int lane = rb_lane(), wave = rb_wave();
  const int net = (int)blockIdx.z & 1, mc = (int)blockIdx.z >> 1;
  const int M = a.m_cnt[net];
  const int m0 = mc * (16 * MT);
  if (m0 >= M) return;                                   // block-uniform
  const int g = (a.n_groups > 1 && (int)blockIdx.x >= a.grp[1].tile_begin) ? 1 : 0;
  const NlRowGroup grp = a.grp[g];
  const int row0 = grp.row_begin + ((int)blockIdx.x - grp.tile_begin) * 16;
  const int row_end = grp.row_begin + grp.row_cnt;
  const NlWeights w = a.w[net];
  const int K = a.K;
  const NlFwdWave wv(K, row0, row_end);
  const int r = wv.r, q = wv.q, lr = wv.lr, lk = wv.lk;
  const rb_buf bmu = rb_make_buf(w.mu), bsg = rb_make_buf(w.sigma), bx = rb_make_buf(a.x);
  float eo2[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) eo2[i] = w.eout[wv.wrow[i]];
  float* wt = &s_wt[wave][0];                             // [16 rows][RB_NL_FWD_WT_LD]
  unsigned xo[MT];
  wv.x_offsets<MT>(grp.x_off, a.rows_total, a.m_base[net], m0, M, xo);
  const unsigned xstep = (unsigned)a.rows_total * 64u;     // bytes between consecutive 16-wide k chunks of the activations
  // the epilogue's bias terms: requested HERE, with the first operands — in the epilogue they were one more dependent round trip
  // at the end of a 4 us chain (the output layer's launch)
  const float b_mu = w.bmu[wv.nb], b_sg = w.bsigma[wv.nb], b_eo = w.eout[wv.nb];

  rb_f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[mt][e] = 0.0f;

  // RING slots of (weights, activations) in flight per wave.  EXACT: no ring slot is ever loaded with a block past the wave's
  // range (the clamped duplicates — the output layer's 2 blocks per wave in a ring of 4, the 3-4 refills of the hidden layer's
  // last round — were a fifth to a half of what a workgroup pulled through its CU: fc_h 15.7 -> 15.0 us, fc_z 6.1 -> 5.1 us; the
  // 64-row form of batch 256 measured 1 us slower with it and keeps the clamped loads)
  constexpr int RING = MT >= 4 ? 3 : 4;
  constexpr bool EXACT = MT <= 2;
  float4 r_mu[RING][2], r_sg[RING][2], r_x[RING][2][MT];
  const int nsc = wv.nsc, b0 = wv.b0;
  {
    const float* ein_g = w.ein + grp.ein_off;
    for (int k4 = (int)threadIdx.x; k4 < (K >> 2); k4 += 64 * RB_NL_FWD_WAVES)
      *reinterpret_cast<float4*>(&s_ein[4 * k4]) = rb_ld4(ein_g + 4 * k4);
  }
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
      for (int mt = 0; mt < MT; ++mt) r_x[d][h][mt] = rb_ld4_buf(bx, xo[mt], so);
    }
  };
#pragma unroll
  for (int d = 0; d < RING; ++d) {
    if (!EXACT) { load_w(d, wv.blk_of(d)); load_x(d, wv.blk_of(d)); }
    else if (d < nsc) { load_w(d, b0 + d); load_x(d, b0 + d); }   // wave-uniform
  }
  __syncthreads();                                       // eps_in visible
  auto stage = [&](int d, int b) {
    const float4 e4 = *reinterpret_cast<const float4*>(&s_ein[b * 32 + 4 * lk]);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      *reinterpret_cast<float4*>(&wt[(8 * i + lr) * RB_NL_FWD_WT_LD + 4 * lk]) = rb_noisy4(r_mu[d][i], r_sg[d][i], eo2[i], e4);
  };
  auto mfmas = [&](int d) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 w4 = *reinterpret_cast<const float4*>(&wt[r * RB_NL_FWD_WT_LD + 16 * h + 4 * q]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = rb_mfma16(r_x[d][h][mt].x, w4.x, acc[mt]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = rb_mfma16(r_x[d][h][mt].y, w4.y, acc[mt]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = rb_mfma16(r_x[d][h][mt].z, w4.z, acc[mt]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = rb_mfma16(r_x[d][h][mt].w, w4.w, acc[mt]);
    }
  };
  // floor(nsc / RING) full rounds without any masking, then a tail that only computes
  const int full = nsc / RING * RING;
  // EXACT: the LAST full round refills only the slots the tail will consume (nsc - full of RING); else every round refills every slot
  const int steady = !EXACT ? full : full >= RING ? full - RING : 0;
  for (int sc0 = 0; sc0 < steady; sc0 += RING) {
#pragma unroll
    for (int d = 0; d < RING; ++d) {
      const int sc = sc0 + d;
      stage(d, b0 + sc);
      load_w(d, wv.blk_of(sc + RING));                   // refill the weight half of this ring slot
      rb_wave_sync();                                    // the tile is private to the wave: LDS executes its ops in order
      mfmas(d);
      load_x(d, wv.blk_of(sc + RING));                   // ... and its activation half, once the MFMAs have read it
      rb_wave_sync();                                    // tile reads done before the next block overwrites it
      RB_SCHED_FENCE();                                  // keep this slot's refill here, not at the end of the loop
    }
  }
  if (steady < full) {                                   // wave-uniform: the last full round
#pragma unroll
    for (int d = 0; d < RING; ++d) {
      const int sc = steady + d;
      const bool refill = sc + RING < nsc;               // wave-uniform
      stage(d, b0 + sc);
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
      stage(d, b0 + full + d);
      rb_wave_sync();
      mfmas(d);
      rb_wave_sync();
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e) s_red[wave][mt * 4 + e][lane] = acc[mt][e];
  __syncthreads();
  for (int idx = (int)threadIdx.x; idx < 4 * MT * 64; idx += 64 * RB_NL_FWD_WAVES) {
    const int slot = idx >> 6, l = idx & 63;
    float v = s_red[0][slot][l];
#pragma unroll
    for (int wi = 1; wi < RB_NL_FWD_WAVES; ++wi) v += s_red[wi][slot][l];
    const int mt = slot >> 2, e = slot & 3;
    const int m = m0 + 16 * mt + 4 * (l >> 4) + e;
    const int n = row0 + (l & 15);
    if (m < M && m < m0 + 16 * MT && n < row_end) {
      float o = v + (b_mu + b_sg * b_eo);                                 // model.py:44 (n == wv.nb for every cell that is stored)
      if (a.relu) o = fmaxf(o, 0.0f);
      const int rowi = a.m_base[net] + m;
      a.out[(int64_t)rowi * a.ld_out + n] = o;
      if (a.out_blocked) a.out_blocked[rb_blocked_index(rowi, n, a.rows_total)] = o;
    }
  }
}
