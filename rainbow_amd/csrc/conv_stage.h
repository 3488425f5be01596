// conv_stage.h — what more than one conv kernel shares: the workgroup size, the geometry of the de-interleaved input patch
// (ConvPatch: SUB, RP, PLANE and the cell function, one constexpr place), the weight-slab staging (rb_wswz, rb_stage_weights_t,
// rb_slab_copy), the f32 patch issue and commit, the u8 -> x/255 unpack, the lazy dY sum and the whole-K 16x16x4 tile (rb_t16_steps).
// Included by conv_fwd.h (for its sections conv_fwd_t16.h, conv_fwd_image.h, conv_fwd_multi.h and conv_fwd_full.h), conv_dx.h and conv_dw.h.
#pragma once
#include "learner_problems.h"

#define RB_CONV_WAVES 8
#define RB_CONV_THREADS (64 * RB_CONV_WAVES)
// bank swizzle of the forward kernels' row-major weight slab (rb_conv_fwd_body): column k of row m
__device__ __forceinline__ int rb_wswz(int m, int k) { return (k & ~3) | ((k & 3) ^ ((m >> 3) & 3)); }
// ---- the weight slab -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rb_st4_t(float* s_w, int q, int m, float4 v) {   // columns 4 q .. 4 q + 3 of row m into s_w[k][33]
  s_w[(4 * q + 0) * 33 + m] = v.x; s_w[(4 * q + 1) * 33 + m] = v.y; s_w[(4 * q + 2) * 33 + m] = v.z; s_w[(4 * q + 3) * 33 + m] = v.w;
}
// weights slab [32 rows starting at row0][K] (row-major, K % 4 == 0) -> s_w[k][33], rows >= rows_valid zeroed,
// rows k in [K, KPAD) zeroed
__device__ __forceinline__ void rb_stage_weights_t(float* s_w, const float* w, int row0, int rows_valid, int K, int KPAD) {
  const int t = (int)threadIdx.x, T = (int)blockDim.x;
  const int lane = t & 63, wave = t >> 6, nw = T >> 6;
  if (K & 3) {                                       // odd history lengths: scalar staging
    for (int m = wave; m < 32; m += nw)
      for (int k = lane; k < K; k += 64) s_w[k * 33 + m] = m < rows_valid ? w[(int64_t)(row0 + m) * K + k] : 0.0f;
  } else {
    // all of a wave's float4 loads are issued before the first LDS store (one memory round trip, not one per row)
    const int kq = K >> 2;
    constexpr int RMAX = 4, QMAX = 4;                // 32 rows / 8 waves, K <= 1024
    float4 v[RMAX][QMAX];
    if (nw * RMAX >= 32 && kq <= 64 * QMAX) {
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {
        const int m = wave + r * nw;
#pragma unroll
        for (int i = 0; i < QMAX; ++i) {
          const int q = lane + 64 * i;
          v[r][i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          if (m < rows_valid && q < kq) v[r][i] = rb_ld4(w + (int64_t)(row0 + m) * K + 4 * q);
        }
      }
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {
        const int m = wave + r * nw;
#pragma unroll
        for (int i = 0; i < QMAX; ++i) {
          const int q = lane + 64 * i;
          if (m < 32 && q < kq) rb_st4_t(s_w, q, m, v[r][i]);
        }
      }
    } else {
      for (int m = wave; m < 32; m += nw) {
        const float* src = w + (int64_t)(row0 + m) * K;
        for (int q = lane; q < kq; q += 64) {
          float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          if (m < rows_valid) x = rb_ld4(src + 4 * q);
          rb_st4_t(s_w, q, m, x);
        }
      }
    }
  }
  for (int e = t; e < (KPAD - K) * 32; e += T) s_w[(K + (e >> 5)) * 33 + (e & 31)] = 0.0f;
}
// row-major weight slab, a straight copy: 32 rows of ROWQ float4s, `src_ld` floats apart in memory, WS floats apart in LDS; rows
// at or beyond rows_valid are zero.  (rb_conv_fwd_body stages the same slab split into issue and commit, with the bank swizzle;
// k_conv_dx_lds's slab is [k'][32], clamped loads: both keep their own loops.)
template <int ROWQ, int WS, int THREADS>
__device__ __forceinline__ void rb_slab_copy(float* s_w, const float* src, int src_ld, int rows_valid, int t) {
  for (int e = t; e < 32 * ROWQ; e += THREADS) {
    const int m = e / ROWQ, q = e - m * ROWQ;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (m < rows_valid) v = rb_ld4(src + (int64_t)m * src_ld + 4 * q);
    rb_st4(s_w + m * WS + 4 * q, v);
  }
}

// ---- the input patch of the forward kernels in LDS ---------------------------------------------------------------------------
// PR rows per channel.  Patch rows are stored DE-INTERLEAVED by stride phase: x -> (x % S) * SUB + x / S, SUB = ceil(IH / S).  The
// lanes of an MFMA operand read are neighbouring output positions, i.e. inputs S apart: in the plain row that is a stride-S access
// (4-way bank conflicts in the first layer, 2-way in the second; the MFMA loop was LDS-bound enough that the two
// first-layer workgroups of a CU stretched each other's staging and epilogue from 1.4 / 2.4 to 4.9 / 4.1 us,
// tools/wg_timeline.py); de-interleaved they are consecutive words.
// CQ = channels per k-slot of a 16x16x4 operand read (0: not a t16 kernel): the channel planes are then padded so that the four
// k-slots (channel groups cin/4 apart) start 16 banks apart.
template <class G_, int PR, int CQ>
struct ConvPatch {
  typedef G_ G;
  static constexpr int SUB = (G::IH + G::S - 1) / G::S;
  static constexpr int RP = G::S * SUB;                    // row pitch (>= IH)
  static_assert((G::OH - 1) + (G::KS - 1) / G::S < SUB, "a tap's positions stay inside their phase's sub-row");
  static constexpr int rb_plane_pad() {
    if (CQ == 0) return 0;
    for (int p = 0; p < 64; p += 2)
      if ((CQ * (PR * RP + p)) % 32 == 16) return p;
    return 0;
  }
  static constexpr int PLANE = PR * RP + rb_plane_pad();   // floats per channel in the patch
  // patch cell of (channel c, element `off` of the channel's [rows][IH] patch)
  static __device__ __forceinline__ int cell(int c, int off) {
    const int r = off / G::IH, x = off - r * G::IH;
    return c * PLANE + r * RP + (x % G::S) * SUB + x / G::S;
  }
};

// An f32 patch through registers: thread t's i-th element is e = i * THREADS + t of the [cin][per_c] patch (per_c = 4 v4) whose rows
// start `row0` floats into each channel plane of xbase.  Issue (global loads into the registers), as quads (IH % 4 == 0) ...
// CLAMP: every load is issued, elements beyond the patch at its last index (k_conv_fwd_multi_t16); otherwise they are skipped
// (ConvFwdBody).  Which of the two a kernel does is its own history: nobody recorded why they differ.
template <class G, bool CLAMP, int N, int THREADS>
__device__ __forceinline__ void rb_patch_issue(float4 (&xv)[N], const float* xbase, int row0, int t, int v4, int total4) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int e = i * THREADS + t;
    if (CLAMP || e < total4) {
      const int ec = (!CLAMP || e < total4) ? e : total4 - 1;
      const int c = ec / v4, q = ec - c * v4;
      xv[i] = rb_ld4(xbase + (int64_t)c * G::IP + row0 + q * 4);
    }
  }
}
// ... or single elements
template <class G, bool CLAMP, int N, int THREADS>
__device__ __forceinline__ void rb_patch_issue(float (&xs)[N], const float* xbase, int row0, int t, int per_c, int total1) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int e = i * THREADS + t;
    if (CLAMP || e < total1) {
      const int ec = (!CLAMP || e < total1) ? e : total1 - 1;
      const int c = ec / per_c, q = ec - c * per_c;
      xs[i] = xbase[(int64_t)c * G::IP + row0 + q];
    }
  }
}
// Commit (the registers to their de-interleaved cells in LDS): quads ...
template <class PG, int N, int THREADS>
__device__ __forceinline__ void rb_patch_commit(float* dst, const float4 (&xv)[N], int t, int v4, int total4) {
  typedef typename PG::G G;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int e = i * THREADS + t;
    if (e < total4) {
      const int c = e / v4, q = e - c * v4;
      if constexpr (G::S == 1) { rb_st4(dst + c * PG::PLANE + q * 4, xv[i]); }       // RP == IH: the quad stays a quad
      else if constexpr (G::S == 2 && (PG::SUB % 2) == 0) {
        // x, x+2 are neighbours of phase 0 and x+1, x+3 of phase 1: two 8-byte stores, lanes 8 bytes apart (conflict-free)
        const int off = q * 4, r = off / G::IH, x = off - r * G::IH;
        float* cell = dst + c * PG::PLANE + r * PG::RP + x / 2;
        *reinterpret_cast<float2*>(cell) = make_float2(xv[i].x, xv[i].z);
        *reinterpret_cast<float2*>(cell + PG::SUB) = make_float2(xv[i].y, xv[i].w);
      } else {
        dst[PG::cell(c, q * 4 + 0)] = xv[i].x; dst[PG::cell(c, q * 4 + 1)] = xv[i].y;
        dst[PG::cell(c, q * 4 + 2)] = xv[i].z; dst[PG::cell(c, q * 4 + 3)] = xv[i].w;
      }
    }
  }
}
// ... or single elements
template <class PG, int N, int THREADS>
__device__ __forceinline__ void rb_patch_commit(float* dst, const float (&xs)[N], int t, int per_c, int total1) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int e = i * THREADS + t;
    if (e < total1) { const int c = e / per_c, q = e - c * per_c; dst[PG::cell(c, q)] = xs[i]; }
  }
}

// u8 frame bytes to exact x/255 (rb_unit): the 4 bytes of a dword, the 16 of a uint4, in memory order
__device__ __forceinline__ void rb_unit4(unsigned w, float* f) {
#pragma unroll
  for (int b = 0; b < 4; ++b) f[b] = rb_unit((uint8_t)((w >> (8 * b)) & 0xFFu));
}
__device__ __forceinline__ void rb_unit16(const uint4& raw, float* f) {
  rb_unit4(raw.x, f); rb_unit4(raw.y, f + 4); rb_unit4(raw.z, f + 8); rb_unit4(raw.w, f + 12);
}

// dY of the last conv layer, never materialised: relu'(mask) times the sum of the hidden layer's `splits` (<= 4) row-split
// partials, in k_dfeat_finish's order ((0 + p0) + p1) + ...
__device__ __forceinline__ float rb_dy_lazy(float mask, const float (&part)[4], int splits) {
  float acc = 0.0f;
#pragma unroll
  for (int sp = 0; sp < 4; ++sp) acc += sp < splits ? part[sp] : 0.0f;
  return mask > 0.0f ? acc : 0.0f;
}

// steps [4 JQ0, 4 JQ1) of a lane's quarter of a whole-K 16x16x4 reduction (lane (x = l & 15, kq = l >> 4): row x of the A slab, rows
// WS apart, its quarter at ap; B cells at the compile-time offsets OFF::at(step) from bp): a ds_read_b128 of the row, four B cells
// at immediate offsets, four MFMAs
template <class OFF, int WS, int JQ0, int JQ1>
__device__ __forceinline__ void rb_t16_steps(const float* ap, const float* bp, rb_f32x4& acc) {
#pragma unroll
  for (int jq = JQ0; jq < JQ1; ++jq) {
    const float4 w4 = rb_ld4(ap + 4 * jq);
    const float b0 = bp[OFF::at(4 * jq + 0)], b1 = bp[OFF::at(4 * jq + 1)], b2 = bp[OFF::at(4 * jq + 2)], b3 = bp[OFF::at(4 * jq + 3)];
    acc = rb_mfma16(w4.x, b0, acc);
    acc = rb_mfma16(w4.y, b1, acc);
    acc = rb_mfma16(w4.z, b2, acc);
    acc = rb_mfma16(w4.w, b3, acc);
  }
}
