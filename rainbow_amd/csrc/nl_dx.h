// nl_dx.h — the NoisyLinear input gradient: dx[m][out_off + k] = sum_{n in rows} dy[m][n] * W[n][k]   (adjoint of the forward).
// Two workgroup bodies, both tenants of the fused backward launch (nl_bwd.h): 64-column tiles with four waves splitting the
// reduction rows, and the tall eight-wave form for the output layer at batch <= 32.
#pragma once
#include "nl_common.h"
#include "kernel_stamp.h"

struct NlDxProblem {
  int row_begin, row_cnt;    // reduction range (weight rows)
  int ein_split_row;         // rows >= this use ein_off1 (fc_h: the advantage stream), else ein_off0
  int ein_off0, ein_off1;
  int out_off;               // column offset in dx
};
struct NlDxArgs {
  const float* dy;           // [M][ldy]
  int ldy, M;
  NlWeights w;
  int K;                     // output columns of one problem
  int n_prob;
  NlDxProblem prob[2];
  int rows_per_split;        // reduction rows per block (multiple of 16); grid.y = splits
  float* out;                // split: part[s][M][ld_out]; else dx[M][ld_out]
  int ld_out;
  const float* mask_src;     // non-split only: dx = mask_src > 0 ? v : 0  (ReLU adjoint), same indexing as out
  // Transposed companions.  dyT [rows][ldyT] (dyT[n][m] == dy[m][n]): when set, the dY operand is read from it — a lane
  // group then reads 16 CONSECUTIVE m of one weight row (64 bytes) instead of 16 addresses a whole dy row (4 KB) apart:
  // the gather made the hidden layer's input gradient 45 us for 1.6 GFLOP at batch 256 (0.23 of f32 MFMA).
  // outT [ld_out][M] (non-split only): the result is ALSO stored transposed, for the next layer's dyT.
  const float* dyT;
  int ldyT;
  float* outT;
};

// the MTC dY operands of a lane for reduction row n (valid: nv) and the m tiles from m0: lane column c of each live tile, else zero
template <int MTC>
__device__ __forceinline__ void rb_nl_dy_tiles(const NlDxArgs& a, int n, bool nv, int m0, int c, int mt_cnt, float (&av)[MTC]) {
#pragma unroll
  for (int mt = 0; mt < MTC; ++mt) {
    const int m = m0 + 16 * mt + c;
    av[mt] = (mt < mt_cnt && nv && m < a.M) ? (a.dyT ? a.dyT[(int64_t)n * a.ldyT + m] : a.dy[(int64_t)m * a.ldy + n]) : 0.0f;
  }
}

// grid = (64-column tiles, row splits, n_prob * m-chunks of 64), block = 256 (4 waves split the rows)
#define RB_NL_DX_LDS (2 * 64 * 64)   // floats: two wave tiles (the four waves meet pairwise, see the reduction below)
// MTC = 16-row m tiles a workgroup can hold (4: 64-row m-chunks; 2: batches of <= 32 — half the accumulators), ST = row-steps of 4
// weight rows whose loads are in flight together.  <2, 8> (batch <= 32): a wave's 64 rows are TWO dependent load ->
// MFMA trips instead of four (round6_wg_timeline_b32.txt: first trip 4.6 us, the three behind it 6.4 of the workgroup's 14.6) —
// the rows enter the accumulators in the same order: an element's bits do not depend on ST.
template <int MTC, int ST>
__device__ __forceinline__ void rb_nl_dx_body(const NlDxArgs& a, int bx, int by, int bz, float* lds) {
  float (*s_red)[64][64] = reinterpret_cast<float (*)[64][64]>(lds);   // [2][64][64]
  const int lane = rb_lane(), wave = rb_wave();
  const int pi = bz % a.n_prob, mc = bz / a.n_prob;
  const NlDxProblem pr = a.prob[pi];
  const int m0 = mc * 64;
  if (m0 >= a.M) return;
  const int mt_cnt0 = (a.M - m0 >= 64) ? 4 : (a.M - m0 + 15) / 16;
  const int mt_cnt = mt_cnt0 < MTC ? mt_cnt0 : MTC;      // (the caller picks MTC >= the launch's m tiles)
  const int K = a.K;
  const int kt = bx * 64;
  const int row_end = pr.row_begin + pr.row_cnt;
  int rb = pr.row_begin + by * a.rows_per_split;
  int re = rb + a.rows_per_split;
  if (re > row_end) re = row_end;
  if (rb >= re) return;                                  // block-uniform
  const int per_wave = (((re - rb) + 3) / 4 + 3) / 4 * 4;  // rows per wave, multiple of 4
  int wr0 = rb + wave * per_wave, wr1 = wr0 + per_wave;
  if (wr1 > re) wr1 = re;

  const int c = lane & 15, q = lane >> 4;
  int col4 = kt + 4 * c;
  if (col4 > K - 4) col4 = K - 4;                        // clamped lanes are never stored
  const float4 e0 = rb_ld4(a.w.ein + pr.ein_off0 + col4);
  const float4 e1 = rb_ld4(a.w.ein + pr.ein_off1 + col4);

  rb_f32x4 acc[MTC][4];
#pragma unroll
  for (int mt = 0; mt < MTC; ++mt)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[mt][j][e] = 0.0f;

  // (staging this workgroup's dY slab in LDS first — row-contiguous loads instead of 16 dy rows per instruction —
  // measured slower: k_nl_bwd 16.7 -> 18.0 us; dY is 128 KB and L1/L2-resident, the extra phase costs more)
#if defined(RB_STAMP)
  const int kid_ = 8 + rb_nl_layer(a.K);
  RB_WGT(kid_, (int)blockIdx.x, 2);
#endif
  for (int nb = wr0; nb < wr1; nb += 4 * ST) {           // ST row-steps of loads in flight per iteration
    float4 w4[ST];
    float av[ST][MTC];
#pragma unroll
    for (int st = 0; st < ST; ++st) {
      const int n = nb + 4 * st + q;
      const bool nv = n < wr1;
      const int nc = nv ? n : wr1 - 1;
      w4[st] = rb_noisy4(rb_ld4(a.w.mu + (int64_t)nc * K + col4), rb_ld4(a.w.sigma + (int64_t)nc * K + col4),
                         a.w.eout[nc], nc >= pr.ein_split_row ? e1 : e0);
      rb_nl_dy_tiles<MTC>(a, n, nv, m0, c, mt_cnt, av[st]);
    }
#pragma unroll
    for (int st = 0; st < ST; ++st) {
      if (nb + 4 * st < wr1) {                             // wave-uniform
#pragma unroll
        for (int mt = 0; mt < MTC; ++mt) {
          if (mt < mt_cnt) {
            acc[mt][0] = rb_mfma16(av[st][mt], w4[st].x, acc[mt][0]);
            acc[mt][1] = rb_mfma16(av[st][mt], w4[st].y, acc[mt][1]);
            acc[mt][2] = rb_mfma16(av[st][mt], w4[st].z, acc[mt][2]);
            acc[mt][3] = rb_mfma16(av[st][mt], w4[st].w, acc[mt][3]);
          }
        }
      }
    }
#if defined(RB_STAMP)
    if (nb == wr0) RB_WGT(kid_, (int)blockIdx.x, 3);
#endif
  }
#if defined(RB_STAMP)
  RB_WGT(kid_, (int)blockIdx.x, 4);
#endif
  // cross-wave sum in a fixed order, (w0 + w2) + (w1 + w3), through two 16 KB tiles instead of four (the LDS footprint
  // sets how many workgroups of the fused backward launch a CU holds)
  if (wave >= 2) {
#pragma unroll
    for (int mt = 0; mt < MTC; ++mt)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < 4; ++j) s_red[wave - 2][(mt * 4 + e) * 4 + j][lane] = acc[mt][j][e];
  }
  __syncthreads();
  if (wave < 2) {
#pragma unroll
    for (int mt = 0; mt < MTC; ++mt)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[mt][j][e] += s_red[wave][(mt * 4 + e) * 4 + j][lane];
  }
  __syncthreads();
  if (wave < 2) {
#pragma unroll
    for (int mt = 0; mt < MTC; ++mt)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < 4; ++j) s_red[wave][(mt * 4 + e) * 4 + j][lane] = acc[mt][j][e];
  }
  __syncthreads();
#if defined(RB_STAMP)
  RB_WGT(kid_, (int)blockIdx.x, 5);
#endif
  const int slots = mt_cnt * 4;                          // (mt, e) pairs; j is the float4 lane
  for (int idx = (int)threadIdx.x; idx < slots * 64; idx += 256) {
    const int slot = idx >> 6, l = idx & 63;
    float4 v;
    float* vv = &v.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = slot * 4 + j;
      vv[j] = s_red[0][s][l] + s_red[1][s][l];
    }
    const int mt = slot >> 2, e = slot & 3;
    const int m = m0 + 16 * mt + 4 * (l >> 4) + e;
    const int k = kt + 4 * (l & 15);
    if (m < a.M && k < K) {
      const int64_t o = ((int64_t)by * a.M + m) * a.ld_out + pr.out_off + k;
      if (a.mask_src) {
        const float4 ms = rb_ld4(a.mask_src + o);
        v.x = ms.x > 0.0f ? v.x : 0.0f;
        v.y = ms.y > 0.0f ? v.y : 0.0f;
        v.z = ms.z > 0.0f ? v.z : 0.0f;
        v.w = ms.w > 0.0f ? v.w : 0.0f;
      }
      rb_st4(a.out + o, v);
      if (a.outT && a.mask_src) {                      // (non-split launches only: block-uniform)
        float* ot = a.outT + (int64_t)(pr.out_off + k) * a.M + m;
        ot[0] = v.x; ot[a.M] = v.y; ot[2 * (int64_t)a.M] = v.z; ot[3 * (int64_t)a.M] = v.w;
      }
    }
  }
}

// Tall form for SMALL weight matrices at batch <= 32 (the output layer: 357 x 512, 1.46 MB of mu | sigma): EIGHT waves per
// workgroup.  With four waves the advantage stream's 306 rows are 80 rows per wave = five dependent load -> MFMA iterations of
// ~1.5 us each (a memory round trip here is ~0.8 us, the 32 MFMAs behind it 0.4 us, nothing overlaps: 8.7 of the workgroup's
// 12.1 us, tools/wg_timeline.py; 16-column tiles on four times the workgroups measured SLOWER — 17 us — their dword loads cost
// more issue than the bytes they save per CU).  Eight waves take 40 rows each in ONE batch of loads: one round trip, 10 MFMAs per
// accumulator chain, then one LDS pass sums the eight partial tiles in wave order.
// A lane holds TWO columns: 32-column tiles, 8-byte loads, still one whole 128-byte line per weight row and row-step — twice the
// workgroups of a 64-column tile at half the bytes each (the advantage stream's 64-column workgroup pulled 157 KB of mu | sigma
// through ONE CU, 8.0 us against the value stream's 5.3).  Every hidden size the streamed kernels accept is a multiple of 32.
// Non-split launches with M <= 32 only; block = 64 * RB_NL_DXT_WAVES threads.
#define RB_NL_DXT_WAVES 8        // (16 waves = 1024 threads cap the kernel at 128 registers: the weight-gradient body of the same launch spilled)
#define RB_NL_DXT_LDS (RB_NL_DXT_WAVES * 32 * 64)
__device__ __forceinline__ float2 rb_ld2(const float* p) { return *reinterpret_cast<const float2*>(p); }
__device__ __forceinline__ void rb_nl_dx_body_tall(const NlDxArgs& a, int bx, int bz, float* lds) {
  float (*s_red)[32][64] = reinterpret_cast<float (*)[32][64]>(lds);   // [waves][(mt * 4 + e) * 4 + j][lane]
  const int lane = rb_lane(), wave = rb_wave();
  const int pi = bz % a.n_prob;
  const NlDxProblem pr = a.prob[pi];
  const int mt_cnt = (a.M + 15) / 16;                     // <= 2
  const int K = a.K;
  const int kt = bx * 32;
  const int row_end = pr.row_begin + pr.row_cnt;
  constexpr int ST = 10;                                  // row-steps of 4 rows in flight per wave: 40 rows
  const int per_wave = ((pr.row_cnt + RB_NL_DXT_WAVES - 1) / RB_NL_DXT_WAVES + 3) / 4 * 4;   // rows per wave, multiple of 4
  const int wr0 = pr.row_begin + wave * per_wave;
  int wr1 = wr0 + per_wave;
  if (wr1 > row_end) wr1 = row_end;
  const int c = lane & 15, q = lane >> 4;
  int col2 = kt + 2 * c;
  if (col2 > K - 2) col2 = K - 2;                        // clamped lanes are never stored
  const float2 e0 = rb_ld2(a.w.ein + pr.ein_off0 + col2);
  const float2 e1 = rb_ld2(a.w.ein + pr.ein_off1 + col2);
  // the ReLU mask of this thread's output cells: requested with the operands (in the epilogue: one more dependent trip)
  constexpr int TT = 64 * RB_NL_DXT_WAVES, EIT = (8 * 64 + TT - 1) / TT;     // 8 (mt, e) slots x 64 lanes over the threads
  float2 msk[EIT];
  int64_t oidx[EIT];
#pragma unroll
  for (int it = 0; it < EIT; ++it) {
    const int idx = (int)threadIdx.x + it * TT;            // slot = idx >> 6 over (mt, e), lane = idx & 63
    const int slot = idx >> 6, l = idx & 63;
    const int m = 16 * (slot >> 2) + 4 * (l >> 4) + (slot & 3);
    int k = kt + 2 * (l & 15);
    if (k > K - 2) k = K - 2;
    oidx[it] = (int64_t)(m < a.M ? m : a.M - 1) * a.ld_out + pr.out_off + k;
    if (a.mask_src) msk[it] = rb_ld2(a.mask_src + oidx[it]);
    else { msk[it].x = 1.0f; msk[it].y = 1.0f; }
  }
  rb_f32x4 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[mt][j][e] = 0.0f;
  for (int nb = wr0; nb < wr1; nb += 4 * ST) {            // (one pass for up to 320 rows per problem)
    float2 w2[ST];
    float av[ST][2];
#pragma unroll
    for (int st = 0; st < ST; ++st) {
      const int n = nb + 4 * st + q;
      const bool nv = n < wr1;
      const int nc = nv ? n : wr1 - 1;
      const float2 mu = rb_ld2(a.w.mu + (int64_t)nc * K + col2), sg = rb_ld2(a.w.sigma + (int64_t)nc * K + col2);
      const float eo = a.w.eout[nc];
      const float2 ei = nc >= pr.ein_split_row ? e1 : e0;
      w2[st].x = rb_noisy1(mu.x, sg.x, eo, ei.x);
      w2[st].y = rb_noisy1(mu.y, sg.y, eo, ei.y);
      rb_nl_dy_tiles<2>(a, n, nv, 0, c, mt_cnt, av[st]);
    }
#pragma unroll
    for (int st = 0; st < ST; ++st) {
      if (nb + 4 * st < wr1) {                             // wave-uniform
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          if (mt < mt_cnt) {
            acc[mt][0] = rb_mfma16(av[st][mt], w2[st].x, acc[mt][0]);
            acc[mt][1] = rb_mfma16(av[st][mt], w2[st].y, acc[mt][1]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int j = 0; j < 2; ++j) s_red[wave][(mt * 4 + e) * 4 + j][lane] = acc[mt][j][e];
  __syncthreads();
#pragma unroll
  for (int it = 0; it < EIT; ++it) {
    const int idx = (int)threadIdx.x + it * TT;
    const int slot = idx >> 6, l = idx & 63;
    if (slot >= mt_cnt * 4) continue;
    float vv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float s = s_red[0][slot * 4 + j][l];
#pragma unroll
      for (int w = 1; w < RB_NL_DXT_WAVES; ++w) s += s_red[w][slot * 4 + j][l];     // fixed order w0, w1, ...
      vv[j] = s;
    }
    const int m = 16 * (slot >> 2) + 4 * (l >> 4) + (slot & 3);
    const int k = kt + 2 * (l & 15);
    if (m < a.M && k < K) {
      float2 v;
      v.x = vv[0]; v.y = vv[1];
      if (a.mask_src) {
        v.x = msk[it].x > 0.0f ? v.x : 0.0f;
        v.y = msk[it].y > 0.0f ? v.y : 0.0f;
      }
      *reinterpret_cast<float2*>(a.out + oidx[it]) = v;
      if (a.outT && a.mask_src) {
        float* ot = a.outT + (int64_t)(pr.out_off + k) * a.M + m;
        ot[0] = v.x; ot[a.M] = v.y;
      }
    }
  }
}
