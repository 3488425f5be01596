// conv_dw.h — the weight-gradient convolution kernel: rb_conv_dw_body (one (image group, position chunk, 32-channel tile) slice per
// workgroup, the 8 waves own disjoint column tiles: no cross-wave reduction) and k_conv_dw_all, which runs every layer's body in one
// launch.  Included by learner_internal.h.
#pragma once
#include "conv_stage.h"
#include "kernel_stamp.h"

// ======================================================================= weight gradient ==
// First-layer weight gradient (the one the generic path is worst at: 12800 reduction positions,
// u8 operand): part[slice][co][col] = sum_{pos in chunk} dY[img][co][pos] * X[img][c][oy*S+ky][ox*S+kx],
// slice = (image, chunk of RC output rows); col == K is the bias column (sum of dY).
// The 8 waves own disjoint 32-wide column tiles of the [32 x K] output, so there is NO cross-wave
// reduction: each wave runs the full position loop for its tile(s) out of LDS.
// grid = (chunks per image, cout / 32, images B); block = 512.
struct ConvLdsDwArgs {
  int cin, cout;
  const float* dy;         // [B][cout][P]
  ImgSrc src;              // FIRST: the state stacks (images [0,B))
  const float* x_f;        // else previous activation [NI][cin][IP], rows [0,B)
  float* part;             // [B * chunks][cout][K+1]
  // dy_splits > 0 (last conv layer): dY = relu'(dy_mask) * sum of dy_splits (<= 4) partials, formed while staging
  const float* dy_part;
  const float* dy_mask;
  int64_t dy_stride;
  int dy_splits;
};

template <class G, int RC, int KMAX>
struct ConvDwLdsSize {
  static constexpr int PC = RC * G::OH;               // positions per chunk
  static constexpr int PCP = (PC + 1) / 2 * 2;        // padded to the MFMA k granule
  static constexpr int PR = (RC - 1) * G::S + G::KS;  // input rows per chunk
  static constexpr int PLANE = PR * G::IH;
  static constexpr int CMAX = KMAX / G::KK;
  static constexpr int FLOATS = PCP * 33 + CMAX * PLANE + PCP + 32;   // dY^T, patch, position offsets, per-image bias sums
};

// ---- stage dY^T (zero beyond the chunk) and the input patch of this image.  Every global load of the dY tile is
// unconditional (clamped address) and issued before the first LDS store: a loop of test-load-store made each of its
// 4-9 iterations a memory round trip.
template <class G, class SZ, bool FIRST>
__device__ __forceinline__ void rb_dw_stage_dy(const ConvLdsDwArgs& a, float* s_a, int img, int co0, int p0, int npos, int t) {
  constexpr int PCP = SZ::PCP;
  constexpr int NIT = (32 * PCP + RB_CONV_THREADS - 1) / RB_CONV_THREADS;
  const int rows_valid = a.cout - co0 < 32 ? a.cout - co0 : 32;
  float v[NIT];
  int off[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int e = t + i * RB_CONV_THREADS;
    int m = e / PCP;
    int p = e - m * PCP;                              // p fastest: coalesced along positions
    if (m > rows_valid - 1) m = rows_valid - 1;
    if (p > npos - 1) p = npos - 1;
    off[i] = (img * a.cout + co0 + m) * G::P + p0 + p;    // 32-bit: B * cout * P floats < 2^31
  }
  bool lazy = false;
  if constexpr (!FIRST) lazy = a.dy_splits > 0;       // block-uniform
  if (lazy) {                                         // (ConvDyLoader of conv_dx.h is the same staging on buffer loads, interior cells only)
    float mv[NIT], pv[NIT][4];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      mv[i] = a.dy_mask[off[i]];
#pragma unroll
      for (int sp = 0; sp < 4; ++sp) pv[i][sp] = a.dy_part[(int64_t)(sp < a.dy_splits ? sp : a.dy_splits - 1) * a.dy_stride + off[i]];
    }
#pragma unroll
    for (int i = 0; i < NIT; ++i) v[i] = rb_dy_lazy(mv[i], pv[i], a.dy_splits);
  } else {
#pragma unroll
    for (int i = 0; i < NIT; ++i) v[i] = a.dy[off[i]];
  }
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int e = t + i * RB_CONV_THREADS;
    const int m = e / PCP, p = e - m * PCP;
    if (e < 32 * PCP) s_a[p * 33 + m] = (p < npos && m < rows_valid) ? v[i] : 0.0f;
  }
}
// ... and its input patch [cin][rows x IH] from input row iy0: u8 frames decoded to exact x/255, or the previous activation
template <class G, class SZ, bool FIRST>
__device__ __forceinline__ void rb_dw_stage_patch(const ConvLdsDwArgs& a, float* s_patch, int img, int rows, int iy0, int t) {
  constexpr int PR = SZ::PR, PLANE = SZ::PLANE;
  const int cin = a.cin;
  if (FIRST) {
    const int per_c = rows * G::IH;
    const int v16 = per_c >> 4;
    const int total16 = cin * v16;
    for (int e0 = 0; e0 < total16; e0 += 2 * RB_CONV_THREADS) {        // both 16-byte loads of a thread are in flight together
      uint4 raw[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int e = e0 + i * RB_CONV_THREADS + t;
        raw[i] = make_uint4(0u, 0u, 0u, 0u);
        if (e < total16) {
          const int c = e / v16, q = e - c * v16;
          const uint8_t* fp = rb_frame_ptr(a.src, img, c, cin, G::IP);
          if (fp) raw[i] = *reinterpret_cast<const uint4*>(fp + iy0 * G::IH + q * 16);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int e = e0 + i * RB_CONV_THREADS + t;
        if (e < total16) {
          const int c = e / v16, q = e - c * v16;
          rb_unit16(raw[i], s_patch + c * PLANE + q * 16);
        }
      }
    }
    const int tail = per_c & 15;
    for (int e = t; e < cin * tail; e += RB_CONV_THREADS) {
      const int c = e / tail, q = (v16 << 4) + e % tail;
      const uint8_t* fp = rb_frame_ptr(a.src, img, c, cin, G::IP);
      s_patch[c * PLANE + q] = fp ? rb_unit(fp[iy0 * G::IH + q]) : 0.0f;
    }
  } else {
    const float* base = a.x_f + (int64_t)img * cin * G::IP;
    const int per_c = rows * G::IH;
    if (PR == G::IH && ((cin * G::IP) & 3) == 0) {
      // the chunk is the whole image (later layers): the patch is one contiguous copy, all of it in flight at once
      constexpr int NV = (SZ::CMAX * PLANE / 4 + RB_CONV_THREADS - 1) / RB_CONV_THREADS;
      const int total4 = (cin * G::IP) >> 2;
      float4 v[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int e = t + i * RB_CONV_THREADS;
        v[i] = rb_ld4(base + 4 * (e < total4 ? e : total4 - 1));
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int e = t + i * RB_CONV_THREADS;
        if (e < total4) { float* d = s_patch + 4 * e; d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w; }
      }
    } else {
      for (int e = t; e < cin * per_c; e += RB_CONV_THREADS) {
        const int c = e / per_c, q = e - c * per_c;
        s_patch[c * PLANE + q] = base[(int64_t)c * G::IP + iy0 * G::IH + q];
      }
    }
  }
}

// body with explicit block coordinates and caller-provided LDS, so several layers can share one launch.
// `grp` = slice index along the image axis: the workgroup sums images [grp * ipb, (grp + 1) * ipb) in registers before
// it writes its slice (ipb = 1 at batch 32; batch 256 uses 8, which keeps the slice count — and the reduction pass
// over the slices — at the batch-32 size).
template <class G, int RC, int KMAX, bool FIRST>
__device__ __forceinline__ void rb_conv_dw_body(const ConvLdsDwArgs& a, int chunk, int cotile, int grp, int nchunks,
                                                int ipb, int batch, float* smem) {
  typedef ConvDwLdsSize<G, RC, KMAX> SZ;
  constexpr int PC = SZ::PC, PCP = SZ::PCP, PR = SZ::PR, PLANE = SZ::PLANE;
  constexpr int TPW = ((KMAX + 31) / 32 + RB_CONV_WAVES - 1) / RB_CONV_WAVES;   // 32-wide column tiles per wave
  float* s_a = smem;                                  // dY^T: [pos][co]
  float* s_patch = smem + PCP * 33;
  int* s_poff = reinterpret_cast<int*>(smem + PCP * 33 + SZ::CMAX * PLANE);
  float* s_bias = smem + PCP * 33 + SZ::CMAX * PLANE + PCP;

  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  constexpr int SBW = 24 + (G::KS == 8 || (G::KS == 5 && G::IH == 84) ? 0 : G::KS == 4 || G::KS == 5 ? 8 : 16);   // RB_STAMP slots
  const bool stamp_me = chunk == 0 && cotile == 0 && grp == 0 && t == 0;
  (void)stamp_me;
#if defined(RB_STAMP)
  if (stamp_me) g_cstamp[SBW + 0] = wall_clock64();
#endif
  const int wgi = (int)blockIdx.x;
  (void)wgi;
  RB_WGT(5, wgi, 0);
  RB_WGT_HW(5, wgi);
  const int co0 = cotile * 32;
  const int cin = a.cin, K = cin * G::KK;
  const int oy0 = chunk * RC;
  const int p0 = oy0 * G::OH;
  int npos = G::P - p0;
  if (npos > PC) npos = PC;
  const int iy0 = oy0 * G::S;
  int rows = G::IH - iy0;
  if (rows > PR) rows = PR;
  const int ntiles = (K + 31) / 32;
  const int kh = lane >> 5, nl = lane & 31;

  for (int p = t; p < PCP; p += RB_CONV_THREADS) {
    const int pc = p < npos ? p : npos - 1;
    s_poff[p] = (pc / G::OH) * G::S * G::IH + (pc % G::OH) * G::S;
  }
  rb_f32x16 acc[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[j][q] = 0.0f;
  float bias_acc = 0.0f;

  for (int ii = 0; ii < ipb; ++ii) {
    const int img = grp * ipb + ii;
    if (img >= batch) break;                          // block-uniform
    if (ii > 0) __syncthreads();                      // the previous image's operands are no longer being read
    rb_dw_stage_dy<G, SZ, FIRST>(a, s_a, img, co0, p0, npos, t);
    rb_dw_stage_patch<G, SZ, FIRST>(a, s_patch, img, rows, iy0, t);
    __syncthreads();
#if defined(RB_STAMP)
    if (stamp_me && ii == 0) g_cstamp[SBW + 1] = wall_clock64();
#endif
    if (ii == 0) { RB_WGT(5, wgi, 1); RB_WGT(5, wgi, 2); RB_WGT(5, wgi, 3); }

    // bias column: sum over the chunk's positions in a fixed order (then over the images, ascending).  Eight lanes per
    // channel take every eighth position and meet through shuffles (lane = 8 * channel-in-wave + part): one thread per
    // channel walking up to 140 dependent LDS reads (~3.7 us) made wave 0 the last wave of every workgroup to finish.
    {
      const int part = lane & 7, ch = (wave << 3) + (lane >> 3);          // 8 waves x 8 channels = 64 slots >= 32 channels
      float sum = 0.0f;
      if (ch < 32)
        for (int p = part; p < npos; p += 8) sum += s_a[p * 33 + ch];
      sum += __shfl_xor(sum, 1, 64);
      sum += __shfl_xor(sum, 2, 64);
      sum += __shfl_xor(sum, 4, 64);
      if (part == 0 && ch < 32 && co0 + ch < a.cout) s_bias[ch] = sum;
    }
    int pofs[PCP / 2];                                  // position offsets of the whole chunk, read once (not per step)
#pragma unroll
    for (int j = 0; j < PCP / 2; ++j) pofs[j] = s_poff[2 * j + kh];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int tile = wave + j * RB_CONV_WAVES;        // wave-uniform
      if (tile < ntiles) {
        int col = tile * 32 + nl;
        if (col > K - 1) col = K - 1;
        const int c = col / G::KK, r = col % G::KK;
        const int koff = c * PLANE + (r / G::KS) * G::IH + (r % G::KS);
#pragma unroll
        for (int jj = 0; jj < PCP / 2; ++jj)
          acc[j] = rb_mfma32(s_a[(2 * jj + kh) * 33 + nl], s_patch[koff + pofs[jj]], acc[j]);
      }
    }
    __syncthreads();                                    // s_bias of this image is complete (and its operands are done with)
    if (t < 32 && co0 + t < a.cout) bias_acc += s_bias[t];
#if defined(RB_STAMP)
    if (stamp_me && ii == 0) g_cstamp[SBW + 2] = wall_clock64();
#endif
    if (ii == 0) RB_WGT(5, wgi, 4);
  }

  float* out = a.part + (((int64_t)grp * nchunks + chunk) * a.cout) * (K + 1);
  if (t < 32 && co0 + t < a.cout) out[(int64_t)(co0 + t) * (K + 1) + K] = bias_acc;
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int tile = wave + j * RB_CONV_WAVES;
    if (tile < ntiles) {
      const bool cv = tile * 32 + nl < K;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = co0 + rb_mfma_row(q, lane);
        if (cv && m < a.cout) out[(int64_t)m * (K + 1) + tile * 32 + nl] = acc[j][q];
      }
    }
  }
#if defined(RB_STAMP)
  if (stamp_me) g_cstamp[SBW + 3] = wall_clock64();
#endif
  RB_WGT(5, wgi, 5);
  RB_WGT(5, wgi, 6);
}

// Every conv layer's weight gradient in ONE launch (they only feed the optimiser and are independent of each other
// once all dact[] exist): block ranges [0,n0) layer 0, [n0,n0+n1) layer 1, ...  Saves two kernel boundaries and fills
// the chip with 288 workgroups instead of 160 + 64 + 64 in sequence.
struct ConvDwAllArgs {
  ConvLdsDwArgs layer[3];
  int nblocks[3];          // workgroups of each layer
  int cotiles[3];
  int batch;
  int ipb[3];              // images summed per workgroup, per layer (the layers' workgroups cost differently: learner_plan.h plan_conv_dw_all)
  int img_fast;            // decode with the image group as the FASTEST index (see ConvLdsFwdArgs::img_fast, conv_fwd.h): needs block ranges and group
                           // counts that are multiples of 8
};
template <class G0, int RC0, class G1, int RC1, int K1, class G2, int RC2, int K2, int NL>
__global__ __launch_bounds__(RB_CONV_THREADS) void k_conv_dw_all(ConvDwAllArgs a) {
  typedef ConvDwLdsSize<G0, RC0, 4 * G0::KK> S0;
  typedef ConvDwLdsSize<G1, RC1, K1> S1;
  typedef ConvDwLdsSize<G2, RC2, K2> S2;
  constexpr int M01 = S0::FLOATS > S1::FLOATS ? S0::FLOATS : S1::FLOATS;
  constexpr int MAXF = (NL > 2 && S2::FLOATS > M01) ? S2::FLOATS : M01;
  __shared__ __attribute__((aligned(16))) float smem[MAXF];
  int b = (int)blockIdx.x;
  if (b < a.nblocks[0]) {                              // decode: chunk fastest, then cout tile, then image
    constexpr int CH = (G0::OH + RC0 - 1) / RC0;
    if (a.img_fast) {
      const int ng = (a.batch + a.ipb[0] - 1) / a.ipb[0], rest = b / ng;
      rb_conv_dw_body<G0, RC0, 4 * G0::KK, true>(a.layer[0], rest % CH, rest / CH, b % ng, CH, a.ipb[0], a.batch, smem);
    } else
    rb_conv_dw_body<G0, RC0, 4 * G0::KK, true>(a.layer[0], b % CH, (b / CH) % a.cotiles[0], b / (CH * a.cotiles[0]), CH, a.ipb[0], a.batch, smem);
    return;
  }
  b -= a.nblocks[0];
  if (b < a.nblocks[1]) {
    constexpr int CH = (G1::OH + RC1 - 1) / RC1;
    if (a.img_fast) {
      const int ng = (a.batch + a.ipb[1] - 1) / a.ipb[1], rest = b / ng;
      rb_conv_dw_body<G1, RC1, K1, false>(a.layer[1], rest % CH, rest / CH, b % ng, CH, a.ipb[1], a.batch, smem);
    } else
    rb_conv_dw_body<G1, RC1, K1, false>(a.layer[1], b % CH, (b / CH) % a.cotiles[1], b / (CH * a.cotiles[1]), CH, a.ipb[1], a.batch, smem);
    return;
  }
  if (NL > 2) {
    b -= a.nblocks[1];
    constexpr int CH = (G2::OH + RC2 - 1) / RC2;
    if (a.img_fast) {
      const int ng = (a.batch + a.ipb[2] - 1) / a.ipb[2], rest = b / ng;
      rb_conv_dw_body<G2, RC2, K2, false>(a.layer[2], rest % CH, rest / CH, b % ng, CH, a.ipb[2], a.batch, smem);
    } else
    rb_conv_dw_body<G2, RC2, K2, false>(a.layer[2], b % CH, (b / CH) % a.cotiles[2], b / (CH * a.cotiles[2]), CH, a.ipb[2], a.batch, smem);
  }
}
