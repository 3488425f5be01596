// act_conv.h — the conv layers of the act path (Agent.act / evaluate_q on ONE un-batched state): one unit of work is one (output
// channel, row group) on the scalar unit rb_act_conv_unit, or one 16-position x 16-channel MFMA tile rb_act_conv_tile at the
// canonical geometries.  The training kernels (conv_fwd.h) are shaped for 96 images: with one image they run 2-3 workgroups per
// layer and cost the same 14 us as with 96 (a pure staging-latency chain).  The units trade that for breadth: hundreds of small
// units of work, so a layer is one memory round trip.  Same arithmetic as model.py:69-72 (f32, fused multiply-add accumulation
// in a fixed order).
// Device functions only: a unit reads its input with agent-coherent loads and stores write-through, so the same body serves a
// launch in which the previous layer was written moments ago by other workgroups (act_path.h k_act_fused, its only caller) and
// a launch of one phase alone.  Included by act_path.h; needs rb_device.h (buffer loads, write-through stores, the MFMA).
#pragma once
#include "rb_common.h"
#include "rb_device.h"

#define RB_ACT_LDS 15360          // floats of input patch per workgroup (60 KB)
#define RB_ACT_MAXPOS 128         // output positions per workgroup (two 64-lane passes)
#define RB_ACT_KMAX 1024          // taps of one output channel (cin * KS * KS)

struct ActConvArgs {
  const float* x;      // [cin][IH][IH]
  const float* w;      // [cout][cin*KS*KS]
  const float* bias;   // [cout]
  float* y;            // [cout][OH*OH]   ReLU applied
  int cin, cout, KS, S, IH, OH, RG;   // RG = output rows per workgroup
};

// One (output channel co, row group from output row oy0) of a conv layer.  All 256 threads of the workgroup call: wave w owns the
// w-th quarter of the reduction, lanes are positions.  s_in [RB_ACT_LDS], s_red [4][RB_ACT_MAXPOS] and s_w [RB_ACT_KMAX] are the
// workgroup's LDS.  The channel's filter goes through LDS (s_w): a scalar load per tap would serialise ~200 cycles of latency per
// tap (measured 15 us).
__device__ __forceinline__ void rb_act_conv_unit(const ActConvArgs& a, int co, int oy0, float* s_in, float (*s_red)[RB_ACT_MAXPOS], float* s_w) {
  const int t = (int)threadIdx.x, lane = t & 63;
  const int wave = rb_wave_uniform(t >> 6);
  int rows = a.OH - oy0;
  if (rows > a.RG) rows = a.RG;
  const int npos = rows * a.OH;
  const int iy0 = oy0 * a.S;
  const int plane = ((rows - 1) * a.S + a.KS) * a.IH;          // staged floats per input channel (whole rows)
  const int total = a.cin * plane;
  const int chan = a.IH * a.IH;
  const rb_buf bx = rb_make_buf(a.x);
  // Staging is ONE memory round trip: every 16-byte load of a thread is issued before the first LDS store (a
  // batch-of-8 dword version took seven dependent round trips: 13.5 us for the 51 KB second-layer input).
  const bool flat = plane == chan;                               // whole image: one contiguous run
  const bool vec = flat ? ((total & 3) == 0) : (((plane | chan | (iy0 * a.IH)) & 3) == 0);
  const int KK = a.KS * a.KS, K = a.cin * KK;
  float wreg[RB_ACT_KMAX / 256];                                  // this thread's taps of the filter: requested with the input
#pragma unroll
  for (int i = 0; i < RB_ACT_KMAX / 256; ++i) {
    const int k = t + 256 * i;
    wreg[i] = a.w[(int64_t)co * K + (k < K ? k : K - 1)];
  }
  if (vec) {
    const int plane4 = plane >> 2, total4 = total >> 2;
    for (int e0 = 0; e0 < total4; e0 += 16 * 256) {
      float4 v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        int e = e0 + i * 256 + t;
        if (e > total4 - 1) e = total4 - 1;
        const int c = flat ? 0 : e / plane4;
        const int q = e - c * plane4;
        v[i] = rb_ld4_buf_sc1(bx, 4u * (unsigned)(c * chan + iy0 * a.IH + 4 * q), 0u);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int e = e0 + i * 256 + t;
        if (e < total4) *reinterpret_cast<float4*>(&s_in[4 * e]) = v[i];
      }
    }
  } else {
    for (int e0 = 0; e0 < total; e0 += 8 * 256) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        int e = e0 + i * 256 + t;
        if (e > total - 1) e = total - 1;
        const int c = e / plane, q = e - c * plane;
        v[i] = rb_ld1_buf_sc1(bx, 4u * (unsigned)(c * chan + iy0 * a.IH + q), 0u);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int e = e0 + i * 256 + t;
        if (e < total) s_in[e] = v[i];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < RB_ACT_KMAX / 256; ++i) {
    const int k = t + 256 * i;
    if (k < K) s_w[k] = wreg[i];
  }
  const int ks = (K + 3) >> 2;
  int k0 = wave * ks, k1 = k0 + ks;
  if (k0 > K) k0 = K;
  if (k1 > K) k1 = K;
  int poff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int p = lane + 64 * j;
    if (p > npos - 1) p = npos - 1;
    poff[j] = (p / a.OH) * a.S * a.IH + (p % a.OH) * a.S;
  }
  __syncthreads();
  float acc[2] = {0.0f, 0.0f};
  int c = k0 / KK, r = k0 - c * KK;
  int ky = r / a.KS, kx = r - ky * a.KS;
#pragma unroll 4
  for (int k = k0; k < k1; ++k) {                               // k, c, ky, kx are wave-uniform (scalar unit)
    const float wv = s_w[k];                                    // LDS broadcast
    const int koff = c * plane + ky * a.IH + kx;
    acc[0] = fmaf(wv, s_in[koff + poff[0]], acc[0]);
    acc[1] = fmaf(wv, s_in[koff + poff[1]], acc[1]);
    if (++kx == a.KS) { kx = 0; if (++ky == a.KS) { ky = 0; ++c; } }
  }
  s_red[wave][lane] = acc[0];
  s_red[wave][lane + 64] = acc[1];
  __syncthreads();
  if (t < npos) {
    const float v = ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t] + a.bias[co];
    rb_st1_wt(a.y, 4u * (unsigned)(co * a.OH * a.OH + oy0 * a.OH + t), fmaxf(v, 0.0f));
  }
  __syncthreads();                                               // s_in / s_red / s_w are reused by the next unit or phase
}

// One 16-position x 16-channel output tile of a conv layer on v_mfma_f32_16x16x4_f32, for the canonical geometries (compile-time
// KS / S / IH / OH / CIN).  The scalar unit above is an LDS-latency chain — per tap one broadcast read, two operand reads and
// two FMAs on ONE wave per SIMD: ~10 us per unit (tools/stamp/act_timeline.py), three quarters of the one-launch path.  Here
// the four waves split K (wave w, k-slot kq: the contiguous sixteenth [(4 w + kq) K / 16, +K / 16) — channel- or row-aligned for
// these geometries, so a step's patch offset is lane base + compile-time constant), 16-36 MFMAs per wave, one LDS sum in
// wave order, bias + ReLU, write-through store.  Stages only the input rows its 16 positions touch.
template <int KS, int S, int IH, int OH, int CIN>
__device__ __forceinline__ void rb_act_conv_tile(const ActConvArgs& a, int pt, int ct, float* smem) {
  constexpr int KK = KS * KS, K = CIN * KK, WS = K + 4, P = OH * OH, KL = K / 16;     // KL = steps per (wave, k-slot)
  static_assert(K % 64 == 0, "whole float4s per k-slot");
  static_assert(((KL % KK) == 0) || ((KK % KL) == 0 && (KL % KS) == 0), "k-slot ranges are channel- or kernel-row-aligned");
  constexpr int RSPAN = (15 + OH - 1) / OH + 1;                 // output rows 16 consecutive positions can touch
  constexpr int NR = (RSPAN - 1) * S + KS;                      // input rows staged (clipped to the image)
  constexpr int PLANE = NR * IH;
  static_assert(16 * WS + CIN * PLANE + 4 * 4 * 64 <= RB_ACT_LDS, "tile operands fit the act path's LDS");
  float* s_wt = smem;                                           // [16][WS]
  float* s_p = smem + 16 * WS;                                  // [CIN][NR][IH]
  float* s_rd = smem + 16 * WS + CIN * PLANE;                   // [4 waves][4][64]
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p0 = pt * 16, co0 = ct * 16;
  const int oy_a = p0 / OH;
  int iy_a = oy_a * S;
  if (iy_a + NR > IH) iy_a = IH - NR;                           // keep the staged window inside the image (NR <= IH)
  const rb_buf bx = rb_make_buf(a.x);
  // ---- every global load of both operands is issued before the first LDS store
  constexpr int WQ = (16 * (K / 4) + 255) / 256;
  float4 wv[WQ];
#pragma unroll
  for (int i = 0; i < WQ; ++i) {
    int e = t + 256 * i;
    if (e > 16 * (K / 4) - 1) e = 16 * (K / 4) - 1;
    const int m = e / (K / 4), q = e - m * (K / 4);
    wv[i] = rb_ld4(a.w + (int64_t)(co0 + m) * K + 4 * q);
  }
  constexpr bool VEC = (IH % 4) == 0;
  constexpr int XN = VEC ? (CIN * PLANE / 4 + 255) / 256 : (CIN * PLANE + 255) / 256;
  float4 xv[VEC ? XN : 1];
  float xs[VEC ? 1 : XN];
#pragma unroll
  for (int i = 0; i < XN; ++i) {
    int e = t + 256 * i;
    if constexpr (VEC) {
      if (e > CIN * PLANE / 4 - 1) e = CIN * PLANE / 4 - 1;
      const int c = e / (PLANE / 4), q = e - c * (PLANE / 4);
      xv[i] = rb_ld4_buf_sc1(bx, 4u * (unsigned)(c * IH * IH + iy_a * IH + 4 * q), 0u);
    } else {
      if (e > CIN * PLANE - 1) e = CIN * PLANE - 1;
      const int c = e / PLANE, q = e - c * PLANE;
      xs[i] = rb_ld1_buf_sc1(bx, 4u * (unsigned)(c * IH * IH + iy_a * IH + q), 0u);
    }
  }
  const int x = lane & 15, kq = lane >> 4;
  float bias4[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bias4[r] = a.bias[co0 + 4 * kq + r];
#pragma unroll
  for (int i = 0; i < WQ; ++i) {
    const int e = t + 256 * i;
    if (e < 16 * (K / 4)) { const int m = e / (K / 4), q = e - m * (K / 4); rb_st4(s_wt + m * WS + 4 * q, wv[i]); }
  }
#pragma unroll
  for (int i = 0; i < XN; ++i) {
    const int e = t + 256 * i;
    if constexpr (VEC) { if (e < CIN * PLANE / 4) rb_st4(s_p + 4 * e, xv[i]); }
    else { if (e < CIN * PLANE) s_p[e] = xs[i]; }
  }
  __syncthreads();
  int p = p0 + x;
  const bool pv = p < P;
  if (p > P - 1) p = P - 1;
  const int k0 = (4 * wave + kq) * KL;                           // first k of this lane's range
  const int c0 = k0 / KK, r0 = k0 % KK;                          // (r0 is a multiple of KS, or 0: the static_assert above)
  const float* bp = s_p + c0 * PLANE + ((p / OH) * S - iy_a + r0 / KS) * IH + (p % OH) * S;
  const float* ap = s_wt + x * WS + k0;
  rb_f32x4 acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = 0.0f;
#pragma unroll
  for (int jq = 0; jq < KL / 4; ++jq) {
    const float4 w4 = rb_ld4(ap + 4 * jq);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = 4 * jq + s;                                  // compile-time after unrolling
      const int off = (j / KK) * PLANE + ((j % KK) / KS) * IH + (j % KK) % KS;
      const float wq = s == 0 ? w4.x : s == 1 ? w4.y : s == 2 ? w4.z : w4.w;
      acc = rb_mfma16(wq, bp[off], acc);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) s_rd[(wave * 4 + r) * 64 + lane] = acc[r];
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                // D[r]: channel 4 kq + r of the tile, position x
      const float v = ((s_rd[(0 * 4 + r) * 64 + lane] + s_rd[(1 * 4 + r) * 64 + lane]) + s_rd[(2 * 4 + r) * 64 + lane]) + s_rd[(3 * 4 + r) * 64 + lane];
      if (pv) rb_st1_wt(a.y, 4u * (unsigned)((co0 + 4 * kq + r) * P + p), fmaxf(v + bias4[r], 0.0f));
    }
  }
  __syncthreads();                                               // the LDS is reused by the next unit or phase
}
// the canonical geometries run on tiles; anything else (the data-efficient stack, other history lengths) on the scalar units
__device__ __forceinline__ int rb_act_conv_tiles(const ActConvArgs& c) {
  const bool ok = (c.KS == 8 && c.S == 4 && c.IH == 84 && c.OH == 20 && c.cin == 4) || (c.KS == 4 && c.S == 2 && c.IH == 20 && c.OH == 9 && c.cin == 32) ||
                  (c.KS == 3 && c.S == 1 && c.IH == 9 && c.OH == 7 && c.cin == 64);
  return (ok && c.cout % 16 == 0) ? ((c.OH * c.OH + 15) / 16) * (c.cout / 16) : 0;
}
__device__ __forceinline__ void rb_act_conv_tile_any(const ActConvArgs& c, int u, float* smem) {
  const int pts = (c.OH * c.OH + 15) / 16;
  if (c.KS == 8) rb_act_conv_tile<8, 4, 84, 20, 4>(c, u % pts, u / pts, smem);
  else if (c.KS == 4) rb_act_conv_tile<4, 2, 20, 9, 32>(c, u % pts, u / pts, smem);
  else rb_act_conv_tile<3, 1, 9, 7, 64>(c, u % pts, u / pts, smem);
}
