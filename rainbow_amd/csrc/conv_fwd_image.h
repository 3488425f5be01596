// conv_fwd_image.h — the one-image forward: rb_conv_fwd_body (a workgroup stages the weight slab and the input patch of one image's
// position chunk, then multiplies) behind k_conv_fwd_lds and k_conv_fwd_t16.  A section of conv_fwd.h.
//
// The body takes explicit block coordinates and caller-provided LDS.
// grid = (position chunks of PCH per image, cout / 32, images), or image-fastest (a.img_fast); block = 64 * ConvFwdWaves::NWV.
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
#pragma once

// ---- rb_conv_fwd_body: what it knows at compile time, what it keeps in registers between issue and commit, its pieces ------------
template <class G_, int NT_, int PR_, int KMAX_, bool FIRST_, int PCH_, bool F32SRC, bool T16_>
struct ConvFwdCfg {
  typedef G_ G;
  typedef ConvFwdLdsSize<G, PR_, KMAX_, T16_> SZ;
  typedef typename SZ::PG PG;
  typedef ConvFwdWaves<KMAX_, PCH_, T16_> WV;
  static constexpr int NT = NT_, PR = PR_, KMAX = KMAX_, PCH = PCH_;
  static constexpr bool FIRST = FIRST_, T16 = T16_;
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
  // input: ONE batch of loads per thread, by kind.  The asserts below hold that a batch covers the patch (cin <= CMAX: the host
  // runs these kernels for history <= 4 only, plan_caps, and the later layers' channel counts are make_layout's constants)
  static constexpr bool x_u8 = FIRST && !F32SRC;
  static constexpr bool x_vec = !x_u8 && (G::IH % 4) == 0;   // then per_c, iy0 * IH and IP are multiples of 4 as well
  // u8 frames, stride-4 geometry (the canonical first layer): DWORD loads — the four bytes of a dword are the four stride
  // phases of one de-interleaved index, so consecutive lanes store consecutive words of each phase's sub-row (conflict-free
  // scalar stores; 16-byte loads put 16-byte-strided lanes on 8 banks)
  static constexpr bool x_dw = x_u8 && G::S == 4 && (G::IH % 4) == 0;
  static constexpr bool x_u16 = x_u8 && !x_dw;               // u8 frames of the other geometries: uint4 loads
  static constexpr int XD = x_dw ? (CMAX * PR * G::IH / 4 + THREADS - 1) / THREADS : 1;
  static constexpr int XU = x_u16 ? 2 : 1, XV = x_vec ? 8 : 1, XS = (!x_u8 && !x_vec) ? 12 : 1;
  static constexpr int NF = x_dw ? XD : XU;                  // frame loads per thread
  // every position chunk's patch (rows [iy0, iy0 + PR) of the input, cut at its last row) is whole uint4s per channel
  static constexpr bool u16_chunks_whole() {
    for (int p0 = 0; p0 < G::P; p0 += PCH) {
      const int iy0 = (p0 / G::OH) * G::S;
      if (((G::IH - iy0 < PR ? G::IH - iy0 : PR) * G::IH) % 16 != 0) return false;
    }
    return true;
  }
  static_assert(!x_u16 || (u16_chunks_whole() && CMAX * (PR * G::IH / 16) <= XU * THREADS), "u8 patch: whole uint4s, one batch of loads");
  static_assert(!x_vec || CMAX * PR * G::IH / 4 <= XV * THREADS, "f32 patch in quads: one batch of loads");
  static_assert(x_u8 || x_vec || CMAX * PR * G::IH <= XS * THREADS, "f32 patch in elements: one batch of loads");
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
  // the input loads: u8 dwords, u8 uint4s, f32 quads, f32 elements (the f32 loads skip elements beyond the patch)
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
      rb_patch_issue<G, false, C::XV, THREADS>(xv, xbase, iy0 * G::IH, t, v4, total4);
    } else {
      rb_patch_issue<G, false, C::XS, THREADS>(xs, xbase, iy0 * G::IH, t, per_c, total1);
    }
  }

  // 3. LDS commit: the tap table (no memory operand) ...
  __device__ __forceinline__ void commit_taps() {
    if constexpr (!C::T16) {
      for (int k = t; k < C::KPAD; k += THREADS) {
        const int kc = k < K ? k : K - 1;
        const int c = kc / G::KK, r = kc % G::KK;
        s_koff[k] = c * C::PLANE + (r / G::KS) * C::RP + ((r % G::KS) % G::S) * C::SUB + (r % G::KS) / G::S;
      }
    }
  }
  // ... the weights ...
  __device__ __forceinline__ void commit_weights() {
    constexpr int WS = C::WS;
    constexpr bool T16 = C::T16;
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
  // ... and the input
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
          const int c = e / v16, q = e - c * v16;         // bytes 16 q .. 16 q + 15 of channel c's patch, decoded
          float f[16];
          rb_unit16(xu[i], f);
#pragma unroll
          for (int b = 0; b < 16; ++b) s_patch[PG::cell(c, q * 16 + b)] = f[b];
        }
      }
    } else if constexpr (C::x_vec) {
      rb_patch_commit<PG, C::XV, THREADS>(s_patch, xv, t, v4, total4);
    } else {
      rb_patch_commit<PG, C::XS, THREADS>(s_patch, xs, t, per_c, total1);
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
    rb_f32x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = 0.0f;
    // the lane's steps [h KQ / 2, (h + 1) KQ / 2) of its quarter: immediates again
    if (kh2 == 0) rb_t16_steps<SZ, SZ::WS, 0, KQ / 8>(L.ap, L.bp, acc);
    else rb_t16_steps<SZ, SZ::WS, KQ / 8, 2 * (KQ / 8)>(L.ap, L.bp, acc);
    float bias1[4];
    rb_t16_bias(a.bias[net], a.cout, cout0 + ct * 16 + 4 * L.kq, bias1);
#pragma unroll
    for (int r = 0; r < 4; ++r) s_part[(tu * 4 + r) * 64 + lane] = acc[r];
    __syncthreads();                                  // (the other waves meet it behind their own epilogue, mfma_t16)
    if (kh2 == 0) {
      rb_f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = rb_t16_half_sum(s_part, tu, r, lane);
      rb_t16_store<G>(a, img, cout0 + ct * 16, L, v, bias1);
    }
    RB_WGT(C::WK, wgi, 4); RB_WGT(C::WK, wgi, 5); RB_WGT(C::WK, wgi, 6);
  }
  __device__ __forceinline__ void mfma_t16() {
    // a wave per (position tile, channel tile)
    constexpr int PT = (C::PCH + 15) / 16, KQ = C::KMAX / 4;
    constexpr bool SPLIT_LAST = C::WV::SPLIT_LAST;
    static_assert(!SPLIT_LAST || C::WV::TILE_WAVES == C::NWV, "SPLIT_LAST: every wave reaches the barrier");
    if (wave >= C::WV::TILE_WAVES) return;   // spare staging waves (no barrier follows)
    if constexpr (SPLIT_LAST) {
      if (wave >= 2 * PT - 2) {                           // wave-uniform: a half-unit
        t16_half_unit();
        return;
      }
    }
    const int pt = wave % PT, ct = wave / PT;               // wave-uniform: position tile, channel tile
    const ConvT16Lane L = rb_t16_lane<G, SZ, C::KMAX, C::PCH>(s_w, s_patch, lane, p0, oy0, pt, ct);
    float bias4[4];
    rb_t16_bias(a.bias[net], a.cout, cout0 + ct * 16 + 4 * L.kq, bias4);
    rb_f32x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = 0.0f;
    rb_t16_steps<SZ, SZ::WS, 0, KQ / 4>(L.ap, L.bp, acc);
    RB_CSTAMP(C::SB + 2);
    RB_WGT(C::WK, wgi, 4);
    rb_t16_store<G>(a, img, cout0 + ct * 16, L, acc, bias4);
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
template <class G, int NT, int PR, int KMAX, bool FIRST, int PCH = 32 * NT, bool F32SRC = false, bool T16 = false>
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
  if constexpr (T16) b.mfma_t16();
  else b.mfma_splitk();
}

// (second launch bound = waves per SIMD: a 512-thread workgroup is 2; 4 where the LDS footprint lets two workgroups share a
// CU — the first layer on u8 frames — so that the register allocation does too; the float-input variant of the acting path
// would spill under that cap, and no kernel of this library may carry a scratch segment)
template <class G, int NT, int PR, int KMAX, bool FIRST, int PCH = 32 * NT, bool F32SRC = false>
__global__ __launch_bounds__(RB_CONV_THREADS, (ConvFwdLdsSize<G, PR, KMAX>::FLOATS * 4 <= 80 * 1024 && !F32SRC) ? 4 : 2) void k_conv_fwd_lds(ConvLdsFwdArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[ConvFwdLdsSize<G, PR, KMAX>::FLOATS];
  if (a.img_fast) rb_conv_fwd_body<G, NT, PR, KMAX, FIRST, PCH, F32SRC>(a, (int)blockIdx.z, (int)blockIdx.y, (int)blockIdx.x, smem);
  else rb_conv_fwd_body<G, NT, PR, KMAX, FIRST, PCH, F32SRC>(a, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, smem);
}

// the t16 variant (rb_conv_fwd_body<..., T16 = true>): grid as k_conv_fwd_lds, block = 64 * ConvFwdWaves<KMAX, PCH, true>::NWV threads
template <class G, int NT, int PR, int KMAX, bool FIRST, int PCH = 32 * NT>
__global__ __launch_bounds__((64 * ConvFwdWaves<KMAX, PCH, true>::NWV))
void k_conv_fwd_t16(ConvLdsFwdArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[ConvFwdLdsSize<G, PR, KMAX, true>::FLOATS + ConvFwdWaves<KMAX, PCH, true>::PARTF];
  if (a.img_fast) rb_conv_fwd_body<G, NT, PR, KMAX, FIRST, PCH, false, true>(a, (int)blockIdx.z, (int)blockIdx.y, (int)blockIdx.x, smem);
  else rb_conv_fwd_body<G, NT, PR, KMAX, FIRST, PCH, false, true>(a, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, smem);
}
