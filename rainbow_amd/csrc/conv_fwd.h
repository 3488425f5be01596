// conv_fwd.h — the forward convolution kernels with LDS-resident operands (model.py:56-58,61-62): rb_conv_fwd_body (one image per
// workgroup; 32x32x2 tiles with the reduction split over 8 waves, or whole-K 16x16x4 tiles) behind k_conv_fwd_lds and k_conv_fwd_t16,
// the image-loop kernels k_conv_fwd_multi_t16 and k_conv_fwd_full, and the helpers only they use (output store, t16 lane setup and
// bias fetch; the whole-K tile itself is rb_t16_steps of conv_stage.h).  Included by learner_internal.h.
//
// At batch 32 the Rainbow conv stack is tiny per image (28 KB of u8 input, <= 51 KB activations,
// <= 147 KB of weights per layer) and the generic implicit GEMM of gemm_core.h spends its time on
// per-element im2col address arithmetic and dependent global loads, not on MFMAs.  Here a
// workgroup stages what it needs ONCE with wide coalesced loads —
//     the input patch of its output positions (u8 frames decoded to exact x/255 on the way in),
//     a 32-channel slab of the weights, transposed to [k][32] so MFMA operand reads are
//     bank-conflict free,
//     a k -> patch-offset table (no div/mod in the inner loop),
// — and then runs a pure LDS -> v_mfma_f32_32x32x2_f32 loop.  The four waves split K; their
// accumulators are reduced through LDS in a fixed order (deterministic) and the epilogue (bias,
// ReLU / ReLU mask) stores rows that are contiguous in the NCHW activation.
#pragma once
#include "conv_stage.h"
#include "kernel_stamp.h"

struct ConvLdsFwdArgs {
  int cin, cout;
  int n_on;                  // images [0,n_on) use net 0, the rest net 1
  const float* w[2];         // [cout][cin*KK]
  const float* bias[2];
  ImgSrc src;                // FIRST layer input
  const float* in_f;         // later layers: [img][cin][IP]
  float* out;                // [img][cout][P]
  float* out_blocked;        // optional second copy of the flattened output in the k-blocked layout of nl_fwd.h
  int rows_total;            //   ... with this many rows (images)
  int ipb;                   // k_conv_fwd_multi_t16 / k_conv_fwd_full: images per workgroup
  int img_fast;              // k_conv_fwd_lds: grid = (images, cout tiles, position chunks) — the image is the fastest block index
};

// one output element (image img, channel m, position p) of a forward epilogue: the NCHW activation and, where asked for, its
// k-blocked copy
template <class G>
__device__ __forceinline__ void rb_conv_store_out(const ConvLdsFwdArgs& a, int img, int m, int p, float o) {
  a.out[((int64_t)img * a.cout + m) * G::P + p] = o;
  if (a.out_blocked) a.out_blocked[rb_blocked_index(img, m * G::P + p, a.rows_total)] = o;   // x.view(-1, conv_output_size), model.py:71
}

// ================================================================================ forward ==
// grid = (position chunks of 32*NT per image, cout / 32, images); block = 256.
// PR = input rows staged per channel (covers the output rows of one position chunk).
// PCH = output positions per workgroup (<= 32 NT; a multiple of the row length keeps the patch at PR rows).
// T16 (the t16 variant below): no reduction scratch, no tap table; the channel planes of the patch are padded (ConvPatch) so that
// the four k-slots of a 16x16x4 operand read (channel groups cin/4 apart) start 16 banks apart.
template <class G, int KMAX, int PLANE, int RP, int SUB>
__device__ __forceinline__ constexpr int rb_t16_off(int j) {            // step j of a lane's K quarter -> offset in the patch
  return (j / G::KK) * PLANE + ((j % G::KK) / G::KS) * RP + (((j % G::KK) % G::KS) % G::S) * SUB + ((j % G::KK) % G::KS) / G::S;
}
template <class G, int NT, int PR, int KMAX, int T16 = 0>
struct ConvFwdLdsSize {
  static constexpr int KGRAN = 2 * RB_CONV_WAVES;
  static constexpr int KPAD = (KMAX + KGRAN - 1) / KGRAN * KGRAN;
  static constexpr int RED = RB_CONV_WAVES * 16 * 64;      // reduction scratch (floats) for ONE 32-position tile, overlays the operands
  // the weight slab keeps its GLOBAL orientation in LDS: 32 rows (output channels) of KPAD + 4 floats.  Staging is then
  // 16-byte loads -> 16-byte LDS stores, conflict-free (the former [k][33] transposed image took 16 scalar stores per
  // thread at 8-way bank conflicts: 1-1.5 us of every workgroup, and it serialised the two first-layer workgroups of a CU —
  // tools/wg_timeline.py: 5.3 us input stage for the second one); the MFMA operand read (lane = row) is 4-way conflicted
  // instead, one read per NT MFMAs, hidden under them.
  static constexpr int WS = KPAD + 4;
  static constexpr int CQ = (KMAX / G::KK) / 4;            // T16: channels per k-slot
  typedef ConvPatch<G, PR, T16 ? CQ : 0> PG;               // the patch: de-interleaved rows, T16: padded planes
  static constexpr int SUB = PG::SUB, RP = PG::RP, PLANE = PG::PLANE;
  static __device__ __forceinline__ constexpr int at(int j) { return rb_t16_off<G, KMAX, PLANE, RP, SUB>(j); }   // rb_t16_steps
  static constexpr int OPS = 32 * WS + (KMAX / G::KK) * PLANE;       // weights then patch, contiguous
  static constexpr int WSZ = T16 ? OPS : (OPS > RED ? OPS : RED);
  static constexpr int FLOATS = WSZ + (T16 ? 0 : KPAD);    // + the tap table (ints)
};
// body with explicit block coordinates and caller-provided LDS, so the layers of the stack can share one launch
// F32SRC (first layer only): the input is a.src.f32 (act / evaluate: float states) instead of the u8 frames.  The kind of
// the input loads is a compile-time property so that only ONE staging register array exists (all three alive at once cost
// the first layer its second workgroup per CU).
// T16: the MFMA phase on v_mfma_f32_16x16x4_f32 with NO split of the reduction: the workgroup has one wave per 16-position x
// 16-channel output tile (PT position tiles x 2 channel tiles = NWV waves), every wave runs the WHOLE K for its tile — no
// cross-wave partial sums, no reduction barriers, the epilogue goes from the accumulators to memory (the cross-wave sum +
// epilogue of the 8-way K split was 2.6 / 1.7 us of the second / third layer's 11.4 / 10.3 us workgroups, profiles/
// round3_final_wg_timeline.txt).  Lane (x = l & 15, kq = l >> 4) owns the CONTIGUOUS quarter [kq K/4, (kq + 1) K/4) of the
// reduction: its A operands are whole float4s of weight row x (one ds_read_b128 per four MFMAs), its B operands are patch
// cells whose offsets are compile-time functions of the step (immediates: no tap table).  Needs cin * KK == KMAX, cin % 4 == 0,
// KMAX % 16 == 0 (host-checked).
template <class G, int NT, int PR, int KMAX, bool FIRST, int PCH = 32 * NT, bool F32SRC = false, int T16 = 0>
struct ConvFwdWaves {
  static constexpr int PT = (PCH + 15) / 16;
  // T16 = channel tiles per wave.  The wave count is rounded up to a multiple of 4 — an even share per SIMD: a 10-wave workgroup
  // puts 3 waves on two SIMDs, and the compiler, which sizes the register allocation for the AVERAGE waves per SIMD its LDS
  // footprint allows (next_free_vgpr is raised to the smallest count that still gives that occupancy), then leaves no room
  // for the second workgroup the LDS would admit (profiles/round4_experiments.txt §5); the spare waves help staging and leave
  // SPLIT_LAST (a wave per (position tile, channel tile) unit, 2 PT = 4 n + 2 units: the first layer's 80-position chunks, ten
  // units): waves w, w + 4, w + 8 share a SIMD, so two SIMDs multiplied for three units and two for two — and with two such
  // workgroups per CU those SIMDs' MFMAs were the launch's critical path.  The last two units run instead as four half-units
  // (unit, reduction half) on four waves, one per SIMD; the halves meet through 4 KB of LDS: 2.5 units per SIMD.
  static constexpr bool SPLIT_LAST = T16 == 1 && PT >= 3 && ((2 * PT) % 4) == 2 && ((KMAX / 4) % 8) == 0;
  static constexpr int TILE_WAVES = T16 == 1 ? (SPLIT_LAST ? 2 * PT + 2 : 2 * PT) : PT;
  static constexpr int PARTF = SPLIT_LAST ? 4 * 4 * 64 : 0;   // floats of LDS behind ConvFwdLdsSize::FLOATS for the half-units' partial tiles
  static constexpr int NWV = T16 == 0 ? RB_CONV_WAVES : (TILE_WAVES + 3) / 4 * 4;
};

// ---- the whole-K 16x16x4 tile of the t16 kernels (rb_conv_fwd_body's T16 section and its half-units, k_conv_fwd_multi_t16) ------
// lane (x = l & 15, kq = l >> 4) of the wave that owns position tile pt and, first, channel tile ct0 of a workgroup at position p0
// (patch rows from output row oy0): its position p (clamped; pv = it is stored), its patch base bp, its weight row ap
struct ConvT16Lane {
  int x, kq, p;
  bool pv;
  const float* bp;
  const float* ap;
};
template <class G, class SZ, int KMAX, int PCH>
__device__ __forceinline__ ConvT16Lane rb_t16_lane(const float* s_w, const float* s_patch, int lane, int p0, int oy0, int pt, int ct0) {
  constexpr int KQ = KMAX / 4, CQ = (KMAX / G::KK) / 4;
  ConvT16Lane L;
  L.x = lane & 15; L.kq = lane >> 4;
  int p = p0 + pt * 16 + L.x;
  L.pv = p < G::P && p < p0 + PCH;
  if (p > G::P - 1) p = G::P - 1;                   // clamped lanes are never stored
  L.p = p;
  L.bp = s_patch + L.kq * CQ * SZ::PLANE + (p / G::OH - oy0) * G::S * SZ::RP + (p % G::OH);
  L.ap = s_w + (ct0 * 16 + L.x) * SZ::WS + L.kq * KQ;
  return L;
}
// the bias terms of a lane's four output channels m0 .. m0 + 3 (D[r]: channel 4 kq + r of the tile)
__device__ __forceinline__ void rb_t16_bias(const float* bias, int cout, int m0, float (&b)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) b[r] = bias[m0 + r < cout ? m0 + r : cout - 1];
}

// ---- rb_conv_fwd_body: what it knows at compile time, what it keeps in registers between issue and commit, its pieces ------------
template <class G_, int NT_, int PR_, int KMAX_, bool FIRST_, int PCH_, bool F32SRC, int T16_>
struct ConvFwdCfg {
  typedef G_ G;
  typedef ConvFwdLdsSize<G, NT_, PR_, KMAX_, T16_> SZ;
  typedef typename SZ::PG PG;
  typedef ConvFwdWaves<G, NT_, PR_, KMAX_, FIRST_, PCH_, F32SRC, T16_> WV;
  static constexpr int NT = NT_, PR = PR_, KMAX = KMAX_, PCH = PCH_, T16 = T16_;
  static constexpr bool FIRST = FIRST_;
  static constexpr int NWV = WV::NWV;
  static constexpr int THREADS = 64 * NWV;
  static constexpr int KPAD = SZ::KPAD;
  static constexpr int SUB = SZ::SUB, RP = SZ::RP, PLANE = SZ::PLANE;      // the patch (ConvPatch)
  static constexpr int CMAX = KMAX / G::KK;
  static_assert(!T16 || (KMAX % 16 == 0 && CMAX % 4 == 0), "t16: whole float4s per k-slot");
  static constexpr int WS = SZ::WS;
  static constexpr int KW = KPAD / RB_CONV_WAVES;            // even, compile-time: the MFMA loop is fully unrolled (not T16)
  static constexpr int HW = KW / 2;
  static constexpr int WR = (32 + NWV - 1) / NWV, WQ = (KMAX + 255) / 256;      // 32 rows over the waves; K <= KMAX: quads of a row per lane
  // input: one batch of loads per thread (every geometry of the two networks fits one batch; more: the loops after it)
  static constexpr bool x_u8 = FIRST && !F32SRC;
  static constexpr bool x_vec = !x_u8 && (G::IH % 4) == 0;   // then per_c, iy0 * IH and IP are multiples of 4 as well
  // u8 frames, stride-4 geometry (the canonical first layer): DWORD loads — the four bytes of a dword are the four stride
  // phases of one de-interleaved index, so consecutive lanes store consecutive words of each phase's sub-row (conflict-free
  // scalar stores; 16-byte loads put 16-byte-strided lanes on 8 banks)
  static constexpr bool x_dw = x_u8 && G::S == 4 && (G::IH % 4) == 0;
  static constexpr int XD = x_dw ? (CMAX * PR * G::IH / 4 + THREADS - 1) / THREADS : 1;
  static constexpr int XU = (x_u8 && !x_dw) ? 2 : 1, XV = x_vec ? 8 : 1, XS = (!x_u8 && !x_vec) ? 12 : 1;
  static constexpr int NF = x_dw ? XD : XU;                  // frame loads per thread
  static constexpr int SB = G::KS == 8 ? 0 : G::KS == 4 ? 8 : 16;    // stamp slots per layer (RB_STAMP builds only)
  static constexpr int WK = FIRST ? 0 : (G::KS == 3 ? 2 : 1);          // timeline id of this layer (RB_STAMP builds only)
};
// the body as an object: the phases are its member functions, what they share its members
template <class C>
struct ConvFwdBody {
  typedef typename C::G G;
  typedef typename C::SZ SZ;
  typedef typename C::PG PG;
  static constexpr int THREADS = C::THREADS;
  const ConvLdsFwdArgs& a;
  // block coordinates and what follows from them
  int t, lane, wave, wgi;
  int img, net, cout0, p0, cin, K, oy0, iy0;
  int rows_valid_w;
  bool w_fast;
  int per_c;                 // elements per channel of the patch (u8: bytes, a 16-byte multiple for the frame geometries)
  int v16, total16, v4, total4, total1;   // ... in uint4s of u8, in float4s (= dwords of u8), and those of all cin channels
  const float* xbase;
  float* smem;
  float* s_w;
  float* s_patch;
  int* s_koff;               // (not T16: no table)
  // the staging registers: global loads land here (issue) and go to LDS later (commit).  Arrays of the kinds that are not
  // compiled in have one element that nothing touches.
  float4 wv[C::WR][C::WQ];
  // zero-copy frames: the window-table entries are REQUESTED first and turned into frame addresses only after the weight
  // loads have been issued (an address formed at once put the table's round trip in front of every other load: 1.5 us
  // from workgroup start to the first weight load, tools/stamp/fine_stage.py)
  int32_t widx[C::NF];
  // (a frame pointer is always one of the kernel's global arguments plus an offset and its validity a flag of its own: with
  // nullptr as the "blank frame" marker the compiler could no longer tell the address space and the first layer's T16
  // instantiation carried six FLAT loads — the library's only ones)
  const uint8_t* fp[C::NF];
  bool fok[C::NF];
  unsigned xd[C::XD];
  uint4 xu[C::XU];
  float4 xv[C::XV];
  float xs[C::XS];

  __device__ __forceinline__ ConvFwdBody(const ConvLdsFwdArgs& a_, int bx, int by, int img_, float* smem_) : a(a_) {
    smem = smem_;
    s_koff = reinterpret_cast<int*>(smem + SZ::WSZ);
    s_w = smem;
    s_patch = smem + 32 * C::WS;
    t = (int)threadIdx.x; lane = t & 63; wave = t >> 6;
    wgi = img_ * 16 + by * 8 + bx;
    img = img_;
    net = img < a.n_on ? 0 : 1;
    cout0 = by * 32;
    p0 = bx * C::PCH;
    cin = a.cin;
    K = cin * G::KK;
    oy0 = p0 / G::OH;
    iy0 = oy0 * G::S;
    int rows = G::IH - iy0;
    if (rows > C::PR) rows = C::PR;
    rows_valid_w = a.cout - cout0 < 32 ? a.cout - cout0 : 32;
    w_fast = (K & 3) == 0 && (K >> 2) <= 64 * C::WQ;
    xbase = C::x_u8 ? nullptr : (C::FIRST ? a.src.f32 + (int64_t)img * cin * G::IP : a.in_f + (int64_t)img * cin * G::IP);
    per_c = rows * G::IH;
    v16 = per_c >> 4; total16 = cin * v16;
    v4 = per_c >> 2; total4 = cin * v4;
    total1 = cin * per_c;
  }

  // 1. weights issue: rb_stage_weights_t's fast path split into issue (loads, here) and commit (LDS stores, commit_weights; cf. rb_slab_copy)
  __device__ __forceinline__ void issue_weights() {
    if (w_fast) {
      const int kq = K >> 2;
#pragma unroll
      for (int r = 0; r < C::WR; ++r) {
        const int m = wave + r * C::NWV;
#pragma unroll
        for (int i = 0; i < C::WQ; ++i) {
          const int q = lane + 64 * i;
          wv[r][i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          if (m < rows_valid_w && q < kq) wv[r][i] = rb_ld4(a.w[net] + (int64_t)(cout0 + m) * K + 4 * q);
        }
      }
    }
  }

  // 2. input issue, by source kind.  u8 frames: the window-table entries are requested in front of the weight loads ...
  __device__ __forceinline__ void request_window() {
    if constexpr (C::x_u8) {
#pragma unroll
      for (int i = 0; i < C::NF; ++i) {
        const int e = i * THREADS + t;
        const int c = C::x_dw ? e / v4 : e / v16;
        widx[i] = -1;
        if ((C::x_dw ? e < total4 : e < total16) && a.src.ring) {
          const int sample = img < a.src.B ? img : (img - a.src.B) % a.src.B;
          widx[i] = a.src.win[(int64_t)sample * a.src.win_len + (img < a.src.B ? c : a.src.n_step + c)];
        }
      }
    }
  }
  // ... and become frame addresses behind them
  __device__ __forceinline__ void frame_ptrs() {
    if constexpr (C::x_u8) {
#pragma unroll
      for (int i = 0; i < C::NF; ++i) {
        const int e = i * THREADS + t;
        const int c = C::x_dw ? e / v4 : e / v16;
        fok[i] = false;
        if (a.src.ring) {
          fp[i] = a.src.ring;
          if (C::x_dw ? e < total4 : e < total16) {
            fok[i] = widx[i] >= 0;
            fp[i] = a.src.ring + (int64_t)(widx[i] < 0 ? 0 : widx[i]) * G::IP;                         // rb_frame_ptr, second half
          }
        } else {
          fp[i] = a.src.u8_states;
          if (C::x_dw ? e < total4 : e < total16) {
            fok[i] = true;
            fp[i] = img < a.src.B ? a.src.u8_states + ((int64_t)img * cin + c) * G::IP
                                     : a.src.u8_next + ((int64_t)((img - a.src.B) % a.src.B) * cin + c) * G::IP;   // rb_frame_ptr, gathered stacks
          }
        }
      }
    }
  }
  // the input loads (first batch): u8 dwords, u8 uint4s, f32 quads, f32 elements.  (The f32 loads skip elements beyond the patch;
  // k_conv_fwd_multi_t16's clamp the index instead.)
  __device__ __forceinline__ void issue_input() {
    frame_ptrs();
    if constexpr (C::x_dw) {
#pragma unroll
      for (int i = 0; i < C::XD; ++i) {
        const int e = i * THREADS + t;
        xd[i] = 0u;
        if (e < total4 && fok[i]) xd[i] = rb_ldg_u32(fp[i] + iy0 * G::IH + 4 * (e - (e / v4) * v4));
      }
    } else if constexpr (C::x_u8) {
#pragma unroll
      for (int i = 0; i < C::XU; ++i) {
        const int e = i * THREADS + t;
        xu[i] = make_uint4(0u, 0u, 0u, 0u);
        if (e < total16 && fok[i]) xu[i] = *reinterpret_cast<const uint4*>(fp[i] + iy0 * G::IH + (e - (e / v16) * v16) * 16);
      }
    } else if constexpr (C::x_vec) {
#pragma unroll
      for (int i = 0; i < C::XV; ++i) {
        const int e = i * THREADS + t;
        if (e < total4) {
          const int c = e / v4, q = e - c * v4;
          xv[i] = rb_ld4(xbase + (int64_t)c * G::IP + iy0 * G::IH + q * 4);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < C::XS; ++i) {
        const int e = i * THREADS + t;
        if (e < total1) {
          const int c = e / per_c, q = e - c * per_c;
          xs[i] = xbase[(int64_t)c * G::IP + iy0 * G::IH + q];
        }
      }
    }
  }

  // 3. LDS commit: the tap table (no memory operand) ...
  __device__ __forceinline__ void commit_taps() {
    if constexpr (C::T16 == 0) {
      for (int k = t; k < C::KPAD; k += THREADS) {
        const int kc = k < K ? k : K - 1;
        const int c = kc / G::KK, r = kc % G::KK;
        s_koff[k] = c * C::PLANE + (r / G::KS) * C::RP + ((r % G::KS) % G::S) * C::SUB + (r % G::KS) / G::S;
      }
    }
  }
  // ... the weights ...
  __device__ __forceinline__ void commit_weights() {
    constexpr int WS = C::WS, T16 = C::T16;
    if (w_fast) {
      const int kq = K >> 2;
#pragma unroll
      for (int r = 0; r < C::WR; ++r) {
        const int m = wave + r * C::NWV;
#pragma unroll
        for (int i = 0; i < C::WQ; ++i) {
          const int q = lane + 64 * i;
          if (q < kq && m < 32) {                                    // rows >= rows_valid were loaded as zeros
            // bank swizzle (rb_wswz): inside its aligned group of four, column k of row m sits at (k & 3) ^ ((m >> 3) & 3) —
            // m >> 3 == r here, a compile-time permutation of the float4
            const float4 v = wv[r][i];
            float4 o;
            if (T16 || (r & 3) == 0) o = v;                          // (r is an unrolled loop index: folded; T16: no swizzle)
            else if ((r & 3) == 1) o = make_float4(v.y, v.x, v.w, v.z);
            else if ((r & 3) == 2) o = make_float4(v.z, v.w, v.x, v.y);
            else o = make_float4(v.w, v.z, v.y, v.x);
            rb_st4(s_w + m * WS + 4 * q, o);
          }
        }
      }
    } else {                                           // odd history lengths: scalar staging
      for (int m = wave; m < 32; m += C::NWV)
        for (int k = lane; k < K; k += 64) s_w[m * WS + (T16 ? k : rb_wswz(m, k))] = m < rows_valid_w ? a.w[net][(int64_t)(cout0 + m) * K + k] : 0.0f;
    }
    for (int e = t; e < (C::KPAD - K) * 32; e += THREADS) s_w[(e & 31) * WS + rb_wswz(e & 31, K + (e >> 5))] = 0.0f;   // columns [K, KPAD)
  }
  __device__ __forceinline__ void put16(int c, int q, const uint4& raw) {   // bytes 16 q .. 16 q + 15 of channel c's patch, decoded
    float f[16];
    rb_unit16(raw, f);
#pragma unroll
    for (int b = 0; b < 16; ++b) s_patch[PG::cell(c, q * 16 + b)] = f[b];
  }
  // ... and the input, with the loads of whatever one batch per thread did not cover
  __device__ __forceinline__ void commit_input() {
    constexpr int PLANE = C::PLANE, RP = C::RP, SUB = C::SUB;
    if constexpr (C::x_dw) {
      constexpr int DPR = G::IH / 4;                       // dwords per input row
#pragma unroll
      for (int i = 0; i < C::XD; ++i) {
        const int e = i * THREADS + t;
        if (e < total4) {
          const int c = e / v4, d = e - c * v4;
          const int r = d / DPR, xi = d - r * DPR;        // bytes 4 xi .. 4 xi + 3 of row r: phases 0..3 of de-interleaved index xi
          float* cell = s_patch + c * PLANE + r * RP + xi;
          float f[4];
          rb_unit4(xd[i], f);
#pragma unroll
          for (int b = 0; b < 4; ++b) cell[b * SUB] = f[b];
        }
      }
    } else if constexpr (C::x_u8) {
#pragma unroll
      for (int i = 0; i < C::XU; ++i) {
        const int e = i * THREADS + t;
        if (e < total16) {
          const int c = e / v16, q = e - c * v16;
          put16(c, q, xu[i]);
        }
      }
      for (int e = C::XU * THREADS + t; e < total16; e += THREADS) {          // beyond one batch (not the frame geometries)
        const int c = e / v16, q = e - c * v16;
        const uint8_t* fr = rb_frame_ptr(a.src, img, c, cin, G::IP);
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (fr) raw = *reinterpret_cast<const uint4*>(fr + iy0 * G::IH + q * 16);
        put16(c, q, raw);
      }
      for (int e = t; e < cin * (per_c & 15); e += THREADS) {   // (no tail for 84-wide frames; kept for generality)
        const int c = e / (per_c & 15), q = (v16 << 4) + e % (per_c & 15);
        const uint8_t* fr = rb_frame_ptr(a.src, img, c, cin, G::IP);
        s_patch[PG::cell(c, q)] = fr ? rb_unit(fr[iy0 * G::IH + q]) : 0.0f;
      }
    } else if constexpr (C::x_vec) {
      rb_patch_commit<PG, C::XV, THREADS>(s_patch, xv, t, v4, total4);
      for (int e = C::XV * THREADS + t; e < total4; e += THREADS) {               // beyond one batch
        const int c = e / v4, q = e - c * v4;
        const float4 v = rb_ld4(xbase + (int64_t)c * G::IP + iy0 * G::IH + q * 4);
        s_patch[PG::cell(c, q * 4 + 0)] = v.x; s_patch[PG::cell(c, q * 4 + 1)] = v.y;
        s_patch[PG::cell(c, q * 4 + 2)] = v.z; s_patch[PG::cell(c, q * 4 + 3)] = v.w;
      }
    } else {
      rb_patch_commit<PG, C::XS, THREADS>(s_patch, xs, t, per_c, total1);
      for (int e = C::XS * THREADS + t; e < total1; e += THREADS) {               // beyond one batch
        const int c = e / per_c, q = e - c * per_c;
        const float v = xbase[(int64_t)c * G::IP + iy0 * G::IH + q];
        s_patch[PG::cell(c, q)] = v;
      }
    }
  }

  // 4. MFMA phase, t16.  A half-unit of SPLIT_LAST (ConvFwdWaves): wave tu of the last four takes reduction half tu >> 1 of unit
  // 2 PT - 2 + (tu & 1); the halves meet through s_part, the first half's wave adds them and stores
  __device__ __forceinline__ void t16_half_unit() {
    constexpr int PT = (C::PCH + 15) / 16, KQ = C::KMAX / 4;
    float* s_part = smem + SZ::FLOATS;                // [half-unit][4][64]
    const int tu = wave - (2 * PT - 2), unit = 2 * PT - 2 + (tu & 1), kh2 = tu >> 1;
    const int upt = unit % PT, ct = unit / PT;
    const ConvT16Lane L = rb_t16_lane<G, SZ, C::KMAX, C::PCH>(s_w, s_patch, lane, p0, oy0, upt, ct);
    rb_f32x4 acc[1];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[0][r] = 0.0f;
    // the lane's steps [h KQ / 2, (h + 1) KQ / 2) of its quarter: immediates again
    if (kh2 == 0) rb_t16_steps<SZ, SZ::WS, 1, 0, KQ / 8>(L.ap, L.bp, acc);
    else rb_t16_steps<SZ, SZ::WS, 1, KQ / 8, 2 * (KQ / 8)>(L.ap, L.bp, acc);
    float bias1[4];
    rb_t16_bias(a.bias[net], a.cout, cout0 + ct * 16 + 4 * L.kq, bias1);
#pragma unroll
    for (int r = 0; r < 4; ++r) s_part[(tu * 4 + r) * 64 + lane] = acc[0][r];
    __syncthreads();                                  // (the other waves meet it behind their own epilogue, mfma_t16)
    if (kh2 == 0) {                                   // first half + second half, bias, ReLU
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = cout0 + ct * 16 + 4 * L.kq + r;
        if (L.pv && m < a.cout)
          rb_conv_store_out<G>(a, img, m, L.p, fmaxf((s_part[(tu * 4 + r) * 64 + lane] + s_part[((tu + 2) * 4 + r) * 64 + lane]) + bias1[r], 0.0f));
      }
    }
    RB_WGT(C::WK, wgi, 4); RB_WGT(C::WK, wgi, 5); RB_WGT(C::WK, wgi, 6);
  }
  __device__ __forceinline__ void mfma_t16() {
    // CTW channel tiles per wave: 1 = a wave per (position tile, channel tile); 2 = a wave per position tile, both channel
    // tiles of the slab from ONE patch operand per step (the first layer: five waves instead of ten per workgroup)
    constexpr int PT = (C::PCH + 15) / 16, KQ = C::KMAX / 4, CTW = C::T16;
    constexpr bool SPLIT_LAST = C::WV::SPLIT_LAST;
    static_assert(!SPLIT_LAST || C::WV::TILE_WAVES == C::NWV, "SPLIT_LAST: every wave reaches the barrier");
    if (wave >= C::WV::TILE_WAVES) return;   // spare staging waves (no barrier follows)
    if constexpr (SPLIT_LAST) {
      if (wave >= 2 * PT - 2) {                           // wave-uniform: a half-unit
        t16_half_unit();
        return;
      }
    }
    const int pt = wave % PT, ct0 = (wave / PT) * CTW;      // wave-uniform: position tile, first channel tile
    const ConvT16Lane L = rb_t16_lane<G, SZ, C::KMAX, C::PCH>(s_w, s_patch, lane, p0, oy0, pt, ct0);
    float bias4[CTW][4];
#pragma unroll
    for (int u = 0; u < CTW; ++u) rb_t16_bias(a.bias[net], a.cout, cout0 + (ct0 + u) * 16 + 4 * L.kq, bias4[u]);
    rb_f32x4 acc[CTW];
#pragma unroll
    for (int u = 0; u < CTW; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[u][r] = 0.0f;
    rb_t16_steps<SZ, SZ::WS, CTW, 0, KQ / 4>(L.ap, L.bp, acc);
    RB_CSTAMP(C::SB + 2);
    RB_WGT(C::WK, wgi, 4);
#pragma unroll
    for (int u = 0; u < CTW; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {                   // D[r]: channel 4 kq + r of the tile, position x
        const int m = cout0 + (ct0 + u) * 16 + 4 * L.kq + r;
        if (L.pv && m < a.cout) rb_conv_store_out<G>(a, img, m, L.p, fmaxf(acc[u][r] + bias4[u][r], 0.0f));
      }
    RB_CSTAMP(C::SB + 3);
    RB_CSTAMP_LAST(C::SB + 5);
    RB_WGT(C::WK, wgi, 5);
    RB_WGT(C::WK, wgi, 6);
    if constexpr (SPLIT_LAST) __syncthreads();            // the split tile's waves exchange their halves behind this barrier
  }

  // 5. MFMA phase, split-K: wave w owns k in [w*KW, (w+1)*KW) of the padded reduction (weights beyond K are zero); cross-wave sum
  __device__ __forceinline__ void mfma_splitk() {
    constexpr int NT = C::NT, KW = C::KW, HW = C::HW, WS = C::WS, RP = C::RP, PCH = C::PCH;
    const int kb = wave * KW;
    int noff[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      int p = p0 + nt * 32 + (lane & 31);
      if (p > G::P - 1) p = G::P - 1;                  // clamped lanes are never stored
      noff[nt] = (p / G::OH - oy0) * G::S * RP + (p % G::OH);        // (de-interleaved rows: neighbouring outputs, neighbouring words)
    }
    rb_f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nt][r] = 0.0f;
    const int kh = lane >> 5, ml = lane & 31;
    float bias_r[(16 * 64) / THREADS];          // the epilogue's bias terms (its rows do not depend on the tile)
#pragma unroll
    for (int it = 0; it < (16 * 64) / THREADS; ++it) {
      const int idx = t + it * THREADS;
      const int m = cout0 + rb_mfma_row(idx >> 6, idx & 63);
      bias_r[it] = a.bias[net][m < a.cout ? m : a.cout - 1];
    }
    // the patch offsets of this wave's k range are read up front: inside the loop they would put an LDS round trip
    // (offset -> operand address) on the critical path of every step (measured 7.1 us of MFMA phase for 5.1 us of MFMAs)
    int kos[HW];
#pragma unroll
    for (int j = 0; j < HW; ++j) kos[j] = s_koff[kb + 2 * j + kh];
    // A operand: row ml, column k = kb + 2 j + kh of the row-major slab.  The row stride is a multiple of 4 (16-byte staging
    // stores), so 32 lanes reading one column would meet in 8 banks, four deep; with the swizzle rows ml, ml + 8, ml + 16, ml + 24
    // keep that column in four different words of its group: conflict-free.  kb % 4 == 0: two lane constants, immediate offsets.
    // (k ranges per wave that are not 4-aligned — the data-efficient first layer, KW = 14 — compute the swizzle per step)
    const int aswz = (ml >> 3) & 3;
    const int a_even = ml * WS + kb + (kh ^ aswz), a_odd = ml * WS + kb + ((2 + kh) ^ aswz);
#pragma unroll
    for (int j = 0; j < HW; ++j) {
      float av;
      if constexpr (KW % 4 == 0) av = s_w[((j & 1) ? a_odd : a_even) + 4 * (j >> 1)];
      else av = s_w[ml * WS + rb_wswz(ml, kb + 2 * j + kh)];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = rb_mfma32(av, s_patch[noff[nt] + kos[j]], acc[nt]);
    }
    RB_CSTAMP(C::SB + 2);
    RB_WGT(C::WK, wgi, 4);
    // cross-wave sum, fixed order w0..w7.  Where the operand area is large enough for the partial sums of ALL NT tiles
    // (the later layers: 2-3 x 32 KB inside 97-118 KB) they are exchanged in one pass — two barriers instead of 2 NT; the
    // first layer keeps one 32 KB tile at a time (its LDS footprint decides how many workgroups share a CU).
    constexpr int EIT = (16 * 64) / THREADS;
    constexpr bool ONEPASS = NT * SZ::RED <= SZ::WSZ;
    constexpr int TP = ONEPASS ? NT : 1;                  // tiles per pass
#pragma unroll
    for (int nt0 = 0; nt0 < NT; nt0 += TP) {
      __syncthreads();                                  // operands (first pass) / the previous pass's sums are no longer read
#pragma unroll
      for (int u = 0; u < TP; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) smem[u * SZ::RED + (wave * 16 + r) * 64 + lane] = acc[nt0 + u][r];
      __syncthreads();
#pragma unroll
      for (int u = 0; u < TP; ++u) {
        const int nt = nt0 + u;
#pragma unroll
        for (int it = 0; it < EIT; ++it) {
          const int idx = t + it * THREADS;
          const int l = idx & 63, r = idx >> 6;
          float v = smem[u * SZ::RED + (0 * 16 + r) * 64 + l];
#pragma unroll
          for (int wv_ = 1; wv_ < RB_CONV_WAVES; ++wv_) v += smem[u * SZ::RED + (wv_ * 16 + r) * 64 + l];
          const int m = cout0 + rb_mfma_row(r, l);
          const int p = p0 + nt * 32 + (l & 31);
          if (m < a.cout && p < G::P && p < p0 + PCH)
            rb_conv_store_out<G>(a, img, m, p, fmaxf(v + bias_r[it], 0.0f));   // (bias fetched before the MFMA loop: a global load
                                                                                  //  here sat on the critical path of every tile's epilogue)
        }
      }
    }
    RB_CSTAMP(C::SB + 3);
    RB_CSTAMP_LAST(C::SB + 5);
    RB_WGT(C::WK, wgi, 5);
    RB_WGT(C::WK, wgi, 6);
  }
};
template <class G, int NT, int PR, int KMAX, bool FIRST, int PCH = 32 * NT, bool F32SRC = false, int T16 = 0>
__device__ __forceinline__ void rb_conv_fwd_body(const ConvLdsFwdArgs& a, int bx, int by, int img, float* smem) {
  typedef ConvFwdCfg<G, NT, PR, KMAX, FIRST, PCH, F32SRC, T16> C;
  ConvFwdBody<C> b(a, bx, by, img, smem);
  RB_CSTAMP(C::SB + 0);
  RB_CSTAMP_LAST(C::SB + 4);
  RB_WGT(C::WK, b.wgi, 0);
  RB_WGT_HW(C::WK, b.wgi);
#if !defined(RB_HOST_INTERP)
  // staging outranks the MFMA phase of a co-resident workgroup: two first-layer workgroups share a CU, and the one that
  // got there second spent 4.4 us converting and storing 7 KB of frames while the first ran its MFMA loop (0.9 us alone;
  // tools/stamp/fine_stage.py) — the wave scheduler favours the older waves.  Dropped again before this workgroup's own MFMAs.
  __builtin_amdgcn_s_setprio(3);
#endif
  // ---- stage: weights (row-major slab into LDS), k -> patch offset table, input patch.
  // Per-workgroup timeline (tools/wg_timeline.py): weights 1.8-2.3 us and input 1.9-3.8 us used to be two memory round
  // trips in sequence (load, store to LDS, load, store to LDS).  Now every global load of BOTH operands is issued before the
  // first LDS store — first-layer frames: the window-table entries first, they gate the frame addresses — and the LDS
  // stores follow in issue order.
  b.request_window();
  b.issue_weights();
  RB_WGT(C::WK, b.wgi, 1);
  RB_WGT(C::WK, b.wgi, 2);
  b.issue_input();
#if defined(RB_STAMP) && defined(RB_STAMP_FINE)
  RB_WGT(C::WK + 4, b.wgi, 0);                               // (fine: loads issued)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  RB_WGT(C::WK + 4, b.wgi, 1);                               // (fine: thread 0's loads have landed)
#endif
  b.commit_taps();
  b.commit_weights();
  b.commit_input();
#if defined(RB_STAMP) && defined(RB_STAMP_FINE)
  RB_WGT(C::WK + 4, b.wgi, 2);                               // (fine: thread 0's LDS stores issued; then the barrier)
#endif
  __syncthreads();
#if !defined(RB_HOST_INTERP)
  __builtin_amdgcn_s_setprio(0);
#endif
  RB_CSTAMP(C::SB + 1);
  RB_WGT(C::WK, b.wgi, 3);
  if constexpr (T16 != 0) b.mfma_t16();
  else b.mfma_splitk();
}

// (second launch bound = waves per SIMD: a 512-thread workgroup is 2; 4 where the LDS footprint lets two workgroups share a
// CU — the first layer on u8 frames — so that the register allocation does too; the float-input variant of the acting path
// would spill under that cap, and no kernel of this library may carry a scratch segment)
template <class G, int NT, int PR, int KMAX, bool FIRST, int PCH = 32 * NT, bool F32SRC = false>
__global__ __launch_bounds__(RB_CONV_THREADS, (ConvFwdLdsSize<G, NT, PR, KMAX>::FLOATS * 4 <= 80 * 1024 && !F32SRC) ? 4 : 2) void k_conv_fwd_lds(ConvLdsFwdArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[ConvFwdLdsSize<G, NT, PR, KMAX>::FLOATS];
  // img_fast: workgroups are spread over the 8 XCDs by linear block index mod 8; with the image as the fastest index (and an
  // image count that is a multiple of 8) every workgroup of image i, in every layer, runs on XCD i mod 8 — the next layer's
  // input is then in that XCD's own L2 instead of behind the fabric
  if (a.img_fast) rb_conv_fwd_body<G, NT, PR, KMAX, FIRST, PCH, F32SRC>(a, (int)blockIdx.z, (int)blockIdx.y, (int)blockIdx.x, smem);
  else rb_conv_fwd_body<G, NT, PR, KMAX, FIRST, PCH, F32SRC>(a, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, smem);
}

// the t16 variant (rb_conv_fwd_body<..., T16 = CTW>): grid as k_conv_fwd_lds, block = 64 * ConvFwdWaves<..., CTW>::NWV threads
template <class G, int NT, int PR, int KMAX, bool FIRST, int PCH = 32 * NT, int CTW = 1>
__global__ __launch_bounds__((64 * ConvFwdWaves<G, NT, PR, KMAX, FIRST, PCH, false, CTW>::NWV))
void k_conv_fwd_t16(ConvLdsFwdArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[ConvFwdLdsSize<G, NT, PR, KMAX, CTW>::FLOATS + ConvFwdWaves<G, NT, PR, KMAX, FIRST, PCH, false, CTW>::PARTF];
  if (a.img_fast) rb_conv_fwd_body<G, NT, PR, KMAX, FIRST, PCH, false, CTW>(a, (int)blockIdx.z, (int)blockIdx.y, (int)blockIdx.x, smem);
  else rb_conv_fwd_body<G, NT, PR, KMAX, FIRST, PCH, false, CTW>(a, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, smem);
}

// ---- large batches, later layers: one weight slab per workgroup, a loop over images around the t16 body -------------------------
// At 768 images the one-image workgroup above stages 34-76 KB of weights for 2.6-5.3 us of MFMAs, 6-15 times per CU.  Here a
// workgroup owns (position chunk, 32-channel slab) and walks a.ipb images.  The workgroup is the t16 body's
// (rb_conv_fwd_body<..., T16 = 1>): one wave per 16-position x 16-channel tile over the WHOLE reduction, the epilogue straight from
// the accumulators — no partial sums, no reduction scratch (a split reduction idles the MFMA pipe during its per-image sums:
// MFMA-busy 0.53-0.57 at batch 256, profiles/round5_sq_counters_*), two barriers per image (patch complete / patch free).  The
// row-major 32-channel slab (and the bias terms) are set up once per net (again where the image range crosses from the online to
// the target net), the next image's patch is in flight (registers) under this image's MFMA loop.  Same LDS image as the one-image
// t16 kernel (117 / 95 KB for the canonical layers 2 / 3).  Needs cin * KK == KMAX, cin % 4 == 0, KMAX % 16 == 0, cout % 32 == 0
// (true of every later layer of the canonical stack).
// grid = (position chunks, cout / 32, image groups) or image-group-fastest (a.img_fast); block = 64 * NWV.
template <class G, int NT, int PR, int KMAX, int PCH = 32 * NT>
__global__ __launch_bounds__((64 * ConvFwdWaves<G, NT, PR, KMAX, false, PCH, false, 1>::NWV))
void k_conv_fwd_multi_t16(ConvLdsFwdArgs a) {
  typedef ConvFwdLdsSize<G, NT, PR, KMAX, 1> SZ;
  typedef ConvFwdWaves<G, NT, PR, KMAX, false, PCH, false, 1> WV;
  constexpr int NWV = WV::NWV, THREADS = 64 * NWV, TILE_WAVES = WV::TILE_WAVES;
  constexpr int WS = SZ::WS, PLANE = SZ::PLANE, CMAX = KMAX / G::KK;
  constexpr int PT = (PCH + 15) / 16, KQ = KMAX / 4;
  static_assert(KMAX % 16 == 0 && CMAX % 4 == 0, "t16: whole float4s per k-slot");
  static_assert(SZ::KPAD == KMAX, "the slab has no padded columns");
  constexpr bool DB = (32 * WS + 2 * CMAX * PLANE) * 4 <= 150 * 1024;      // room for a second patch buffer
  __shared__ __attribute__((aligned(16))) float smem[SZ::FLOATS + (DB ? CMAX * PLANE : 0)];
  float* s_w = smem;
  float* s_patch = smem + 32 * WS;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int img0 = (a.img_fast ? (int)blockIdx.x : (int)blockIdx.z) * a.ipb;
  const int img_end = img0 + a.ipb < a.rows_total ? img0 + a.ipb : a.rows_total;
  const int cout0 = (int)blockIdx.y * 32;
  const int p0 = (a.img_fast ? (int)blockIdx.z : (int)blockIdx.x) * PCH;
  const int cin = a.cin;                              // == CMAX
  const int oy0 = p0 / G::OH;
  const int iy0 = oy0 * G::S;
  int rows = G::IH - iy0;
  if (rows > PR) rows = PR;
  const int per_c = rows * G::IH;
  // ---- the patch of one image: loads into registers (issue), de-interleaved LDS stores later (commit): rb_conv_fwd_body's f32 paths
  constexpr bool x_vec = (G::IH % 4) == 0;
  constexpr int XV = x_vec ? (CMAX * PR * G::IH / 4 + THREADS - 1) / THREADS : 1;
  constexpr int XS = x_vec ? 1 : (CMAX * PR * G::IH + THREADS - 1) / THREADS;
  const int v4 = per_c >> 2, total4 = cin * v4, total1 = cin * per_c;
  float4 xv[XV];
  float xs[XS];
  auto issue = [&](int img) {                         // (every load is issued, at a clamped index; ConvFwdBody::issue_input skips instead)
    const float* xbase = a.in_f + (int64_t)img * cin * G::IP;
    if constexpr (x_vec) {
#pragma unroll
      for (int i = 0; i < XV; ++i) {
        const int e = i * THREADS + t;
        const int ec = e < total4 ? e : total4 - 1;
        const int c = ec / v4, q = ec - c * v4;
        xv[i] = rb_ld4(xbase + (int64_t)c * G::IP + iy0 * G::IH + q * 4);
      }
    } else {
#pragma unroll
      for (int i = 0; i < XS; ++i) {
        const int e = i * THREADS + t;
        const int ec = e < total1 ? e : total1 - 1;
        const int c = ec / per_c, q = ec - c * per_c;
        xs[i] = xbase[(int64_t)c * G::IP + iy0 * G::IH + q];
      }
    }
  };
  auto commit = [&](float* dst) {
    if constexpr (x_vec) rb_patch_commit<typename SZ::PG, XV, THREADS>(dst, xv, t, v4, total4);
    else rb_patch_commit<typename SZ::PG, XS, THREADS>(dst, xs, t, per_c, total1);
  };
  // ---- this wave's tile (rb_conv_fwd_body, T16 section): position tile pt, channel tile ct0; lane (x, kq)
  const bool tile_wave = wave < TILE_WAVES;
  const int pt = wave % PT, ct0 = (wave / PT) % 2;
  const ConvT16Lane L = rb_t16_lane<G, SZ, KMAX, PCH>(s_w, s_patch, lane, p0, oy0, pt, ct0);
  float bias4[4] = {0.0f, 0.0f, 0.0f, 0.0f};

  auto stage_slab = [&](int img) {                    // the slab (row-major, WS apart) and the bias terms of image img's net
    const int net = img < a.n_on ? 0 : 1;
    rb_slab_copy<KMAX / 4, WS, THREADS>(s_w, a.w[net] + (int64_t)cout0 * KMAX, KMAX, a.cout - cout0 < 32 ? a.cout - cout0 : 32, t);
    rb_t16_bias(a.bias[net], a.cout, cout0 + ct0 * 16 + 4 * L.kq, bias4);
  };
  auto tile = [&](int img, const float* bpi) {        // this wave's tile of image img from the patch bpi points into: MFMAs + epilogue
    rb_f32x4 acc[1];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[0][r] = 0.0f;
    rb_t16_steps<SZ, SZ::WS, 1, 0, KQ / 4>(L.ap, bpi, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {                     // D[r]: channel 4 kq + r of the tile, position x
      const int m = cout0 + ct0 * 16 + 4 * L.kq + r;
      if (L.pv && m < a.cout) rb_conv_store_out<G>(a, img, m, L.p, fmaxf(acc[0][r] + bias4[r], 0.0f));
    }
  };

  issue(img0);
  if constexpr (DB) {
    // TWO patch buffers (they fit beside the slab: the third canonical layer): image i + 1's patch is written to the other buffer
    // at the START of iteration i — its LDS stores overlap the first MFMAs of image i — and image i + 2's loads are requested right
    // behind it; ONE barrier per image (patch i + 1 complete, patch i free).
    stage_slab(img0);
    commit(s_patch);
    __syncthreads();                                  // (the slab's stores and the first patch: once)
    if (img0 + 1 < img_end) issue(img0 + 1);
    int cur = 0;
    for (int img = img0; img < img_end; ++img) {
      if (img != img0 && img == a.n_on) {             // block-uniform: the net changes inside this group (every wave is past the barrier)
        stage_slab(img);
        __syncthreads();
      }
      if (img + 1 < img_end) {
        commit(s_patch + (cur ^ 1) * (CMAX * PLANE));
        if (img + 2 < img_end) issue(img + 2);
      }
      if (tile_wave) tile(img, L.bp + cur * (CMAX * PLANE));
      __syncthreads();
      cur ^= 1;
    }
  } else {
    // RB_STAMP builds (tools/wg_timeline.py, kernel id = layer): slot 0 start, 1 / 3 the first / second image's patch (and slab)
    // complete, 2 / 4 its tiles done, 6 end
    const int wgt = (int)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z));
    constexpr int WKM = G::KS == 4 ? 1 : 2;
    (void)wgt; (void)WKM;
    RB_WGT(WKM, wgt, 0);
    for (int img = img0; img < img_end; ++img) {
      if (img == img0 || img == a.n_on) stage_slab(img);   // block-uniform (every wave is past the previous image's MFMA loop: the barrier below)
      commit(s_patch);
      __syncthreads();                                // patch (and slab) complete
      if (img == img0) RB_WGT(WKM, wgt, 1);
      if (img == img0 + 1) RB_WGT(WKM, wgt, 3);
      if (img + 1 < img_end) issue(img + 1);
      if (tile_wave) tile(img, L.bp);                 // wave-uniform; the spare waves (NWV is a multiple of 4) only stage
      __syncthreads();                                // every wave is done reading this image's patch (and, at a net change, the slab)
      if (img == img0) RB_WGT(WKM, wgt, 2);
      if (img == img0 + 1) RB_WGT(WKM, wgt, 4);
    }
    RB_WGT(WKM, wgt, 5);
    RB_WGT(WKM, wgt, 6);
  }
}

// ---- large batches, FIRST layer: whole image per workgroup, no split of the reduction ---------------------------
// The first layer's reduction is short (K = 256): splitting it over 8 waves leaves 16 MFMA steps per wave and tile, and
// the cross-wave sum + barriers cost as much as the MFMAs (measured 2.7 us of 5.6 per 80-position chunk).  Here the whole
// image (cin planes, decoded to f32) and the 32-channel slab sit in LDS (113 + 34 KB), every wave owns whole 32-position
// tiles (wave w: tiles w and w + 8) and runs the full reduction for them: no partial sums, no scratch, the epilogue
// goes from the accumulators to memory.  A workgroup walks a.ipb images of one net; the next image's frames are in
// flight under the MFMA loop.
// grid = (1, 1, image groups); block = 512.  Requires cout <= 32, cin * KK == KMAX, u8 frames.
template <class G>
__device__ __forceinline__ constexpr int rb_patch_off(int k) {           // reduction index (c, ky, kx) -> offset in the image planes
  return (k / G::KK) * G::IP + ((k % G::KK) / G::KS) * G::IH + (k % G::KK) % G::KS;
}
template <class G, int KMAX>
struct ConvFwdFullLds {
  static constexpr int KPAD = (KMAX + 1) / 2 * 2;
  static constexpr int CMAX = KMAX / G::KK;
  static constexpr int NTILES = (G::P + 31) / 32;
  // TAIL16: the last 32-position tile holds at most 16 positions and 12 full tiles precede it (the canonical first layer: 400 =
  // 12 * 32 + 16).  As a 13th 32x32 tile it gave ONE SIMD four tiles and the others three (waves w and w + 4 share a SIMD).  It
  // runs instead as four 16x16x4 units — (channel half, reduction half), one on each of waves 4..7, i.e. one per SIMD — whose
  // two reduction halves meet through 4 KB of LDS behind the end-of-image barrier: 3.25 tiles per SIMD instead of 4 / 3 / 3 / 3.
  static constexpr bool TAIL16 = (G::P % 32) != 0 && (G::P % 32) <= 16 && NTILES == 13 && RB_CONV_WAVES == 8 && (G::KS % 4) == 0 && (CMAX % 2) == 0;
  static constexpr int TAILF = TAIL16 ? 4 * 4 * 64 : 0;
  static constexpr int FLOATS = KPAD * 33 + CMAX * G::IP + TAILF;
  static constexpr bool FITS = FLOATS * 4 <= 160 * 1024 && NTILES <= 2 * RB_CONV_WAVES && (G::IP % 16) == 0;
};
// the 32x32x2 tiles of a wave (NA of them, patch offsets noff[]) over the WHOLE reduction.  Tap offsets are compile-time functions
// of the step (no table: a table read per step put two dependent LDS round trips in front of every MFMA — measured 38 us per
// image for 13 us of MFMAs); K == KMAX (host-checked): straight-line code the compiler can pipeline
template <class G, int CMAX, int KPAD, int NA>
__device__ __forceinline__ void rb_full_tiles(const float* s_w, const float* s_patch, const int (&noff)[2], int kh, int ml, rb_f32x16 (&acc)[2]) {
  if constexpr (G::KS % 2 == 0) {
    // even kernel sizes: the two taps of a step are neighbours (kx, kx + 1) — the lane's half goes into the base
    // pointers, a step's offsets are immediates, and the channel loop only advances the bases (a fully unrolled
    // 128-step body needed a base register per 1 KB window of ds_read2: 255 VGPRs and a scratch segment)
    const float* pb0 = s_patch + noff[0] + kh;
    const float* pb1 = s_patch + noff[1] + kh;      // (NA == 1: not read)
    const float* wp = s_w + kh * 33 + ml;
#pragma unroll 1
    for (int c = 0; c < CMAX; ++c) {
#pragma unroll
      for (int jj = 0; jj < G::KK / 2; ++jj) {
        const float av = wp[2 * jj * 33];
        acc[0] = rb_mfma32(av, pb0[rb_patch_off<G>(2 * jj)], acc[0]);
        if constexpr (NA == 2) acc[1] = rb_mfma32(av, pb1[rb_patch_off<G>(2 * jj)], acc[1]);
      }
      pb0 += G::IP; pb1 += G::IP; wp += G::KK * 33;
    }
  } else {
    // odd sizes: a step's two taps can sit in different rows or planes — select between two constants
#pragma unroll
    for (int j = 0; j < KPAD / 2; ++j) {
      const int o = kh ? rb_patch_off<G>(2 * j + 1) : rb_patch_off<G>(2 * j);
      const float av = s_w[(2 * j + kh) * 33 + ml];
#pragma unroll
      for (int u = 0; u < NA; ++u) acc[u] = rb_mfma32(av, s_patch[noff[u] + o], acc[u]);
    }
  }
}
template <class G, int KMAX>
__global__ __launch_bounds__(RB_CONV_THREADS) void k_conv_fwd_full(ConvLdsFwdArgs a) {
  typedef ConvFwdFullLds<G, KMAX> SZ;
  constexpr int KPAD = SZ::KPAD, CMAX = SZ::CMAX, NTILES = SZ::NTILES;
  __shared__ __attribute__((aligned(16))) float s_all[SZ::FLOATS];
  float* s_w = s_all;
  float* s_patch = s_all + KPAD * 33;
  float* s_tail = s_all + KPAD * 33 + CMAX * G::IP;    // TAIL16: [unit][4][64] partial tiles
  (void)s_tail;
  constexpr bool TAIL16 = SZ::TAIL16;
  constexpr int FT = TAIL16 ? NTILES - 1 : NTILES;     // tiles that run as 32x32 tiles

  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
#if defined(RB_STAMP)
  const bool fst = G::KS == 8 && t == 0 && blockIdx.z == 0;
#define RB_FSTAMP(i) do { if (fst) g_cstamp[i] = wall_clock64(); } while (0)
#else
#define RB_FSTAMP(i) ((void)0)
#endif
  RB_FSTAMP(48);
  // images [z * ipb, (z + 1) * ipb) of the whole list (net 0's images first): a workgroup whose range straddles the two
  // nets re-stages the weight slab once — uniform groups keep 768 images at exactly 3 per workgroup on 256 CUs
  const int img0 = (int)blockIdx.z * a.ipb;
  const int img_end = img0 + a.ipb < a.rows_total ? img0 + a.ipb : a.rows_total;
  const int cin = a.cin;
  const int K = cin * G::KK;

  // frames of one image: 16-byte loads into registers (issue), decoded to exact x/255 into LDS later (commit)
  constexpr int V16 = G::IP / 16;
  constexpr int NU = (CMAX * V16 + RB_CONV_THREADS - 1) / RB_CONV_THREADS;
  uint4 pu[NU];
  const int total16 = cin * V16;
  auto issue = [&](int img) {
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int e = i * RB_CONV_THREADS + t;
      pu[i] = make_uint4(0u, 0u, 0u, 0u);
      if (e < total16) {
        const int c = e / V16, q = e - c * V16;
        const uint8_t* fp = rb_frame_ptr(a.src, img, c, cin, G::IP);
        if (fp) pu[i] = *reinterpret_cast<const uint4*>(fp + q * 16);
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int e = i * RB_CONV_THREADS + t;
      if (e < total16) rb_unit16(pu[i], s_patch + e * 16);   // planes are contiguous: c * IP + q * 16
    }
  };

  const int kh = lane >> 5, ml = lane & 31;
  const bool two = wave + RB_CONV_WAVES < FT;                           // wave-uniform: a second tile
  // TAIL16 unit of waves 4..7: channel half ct, reduction half kh2; lane (x, kq) = (position / channel row, k slot)
  const int tu = wave - 4, tct = tu & 1, tkh = (tu >> 1) & 1, tx = lane & 15, tkq = lane >> 4;
  float tbias[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  (void)tct; (void)tkh; (void)tx; (void)tkq;
  int noff[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    int p = (wave + u * RB_CONV_WAVES) * 32 + ml;
    if (p > G::P - 1) p = G::P - 1;                  // clamped lanes are never stored
    noff[u] = (p / G::OH) * G::S * G::IH + (p % G::OH) * G::S;
  }
  float bias_r[16];

  issue(img0);
  for (int img = img0; img < img_end; ++img) {
    if (img == img0 || img == a.n_on) {               // block-uniform: (re)stage the slab and bias of this image's net
      const int net = img < a.n_on ? 0 : 1;           // (every wave has passed the end-of-image barrier: s_w is idle)
      rb_stage_weights_t(s_w, a.w[net], 0, a.cout < 32 ? a.cout : 32, K, KPAD);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = rb_mfma_row(r, lane);
        bias_r[r] = a.bias[net][m < a.cout ? m : a.cout - 1];
      }
      if constexpr (TAIL16) rb_t16_bias(a.bias[net], a.cout, tct * 16 + 4 * tkq, tbias);
    }
    RB_FSTAMP(img == img0 ? 57 : 58);
    commit();
    RB_FSTAMP(img == img0 ? 59 : 60);
    __syncthreads();            // image complete (first image: weights and tap table as well)
    RB_FSTAMP(img == img0 ? 49 : img == img0 + 1 ? 53 : 61);
    if (img + 1 < img_end) issue(img + 1);
    rb_f32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][r] = 0.0f; acc[1][r] = 0.0f; }
    if (two) rb_full_tiles<G, CMAX, KPAD, 2>(s_w, s_patch, noff, kh, ml, acc);
    else rb_full_tiles<G, CMAX, KPAD, 1>(s_w, s_patch, noff, kh, ml, acc);
    if constexpr (TAIL16) {
      if (wave >= 4) {                                  // wave-uniform
        constexpr int CH = CMAX / 2;                    // channels per reduction half
        int p = (NTILES - 1) * 32 + tx;
        if (p > G::P - 1) p = G::P - 1;                 // clamped lanes are never stored
        // k = c * KK + 4 j + kq: KS % 4 == 0, so the slot kq stays inside a kernel row — it goes into the base pointers and a
        // step's offsets are immediates, as in the 32x32 loops (rb_full_tiles)
        const float* pb = s_patch + tkh * CH * G::IP + (p / G::OH) * G::S * G::IH + (p % G::OH) * G::S + tkq;
        const float* wp = s_w + (tkh * CH * G::KK + tkq) * 33 + tct * 16 + tx;
        rb_f32x4 tacc;
#pragma unroll
        for (int r = 0; r < 4; ++r) tacc[r] = 0.0f;
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
          for (int j = 0; j < G::KK / 4; ++j)
            tacc = rb_mfma16(wp[(c * G::KK + 4 * j) * 33], pb[c * G::IP + rb_patch_off<G>(4 * j)], tacc);
#pragma unroll
        for (int r = 0; r < 4; ++r) s_tail[(tu * 4 + r) * 64 + lane] = tacc[r];
      }
    }
    RB_FSTAMP(img == img0 ? 50 : 54);
    // epilogue straight from the accumulators: row r of the tile is output channel rb_mfma_row(r, lane), 32 consecutive
    // positions per half-wave (contiguous in the NCHW activation)
    float* outi = a.out + (int64_t)img * a.cout * G::P;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = rb_mfma_row(r, lane);
      const int p0 = wave * 32 + ml;
      if (m < a.cout && p0 < G::P) outi[m * G::P + p0] = fmaxf(acc[0][r] + bias_r[r], 0.0f);
      const int p1 = (wave + RB_CONV_WAVES) * 32 + ml;
      if (two && m < a.cout && p1 < G::P) outi[m * G::P + p1] = fmaxf(acc[1][r] + bias_r[r], 0.0f);
    }
    RB_FSTAMP(img == img0 ? 51 : 55);
    __syncthreads();            // every wave is done reading this image before the next one is committed
    if constexpr (TAIL16) {
      // the tail tile: reduction half 0 + half 1 (fixed order), bias, ReLU — waves 4 and 5, one channel half each.  The scratch
      // is written again only behind the next image's commit barrier.
      if (wave == 4 || wave == 5) {
        const int p = (NTILES - 1) * 32 + tx;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = tct * 16 + 4 * tkq + r;
          const float v = s_tail[(tu * 4 + r) * 64 + lane] + s_tail[((tu + 2) * 4 + r) * 64 + lane];
          if (m < a.cout && p < G::P) outi[m * G::P + p] = fmaxf(v + tbias[r], 0.0f);
        }
      }
    }
    RB_FSTAMP(img == img0 ? 52 : 56);
  }
}
