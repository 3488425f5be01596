// conv_fwd_full.h — large batches, FIRST layer: k_conv_fwd_full, whole image per workgroup, no split of the reduction, and its LDS
// sizing ConvFwdFullLds (the launch plan asks it whether a geometry FITS).  A section of conv_fwd.h.
//
// The first layer's reduction is short (K = 256): splitting it over 8 waves leaves 16 MFMA steps per wave and tile, and
// the cross-wave sum + barriers cost as much as the MFMAs (measured 2.7 us of 5.6 per 80-position chunk).  Here the whole
// image (cin planes, decoded to f32) and the 32-channel slab sit in LDS (113 + 34 KB), every wave owns whole 32-position
// tiles (wave w: tiles w and w + 8) and runs the full reduction for them: no partial sums, no scratch, the epilogue
// goes from the accumulators to memory.  A workgroup walks a.ipb images of one net; the next image's frames are in
// flight under the MFMA loop.
// grid = (1, 1, image groups); block = 512.  Requires cout <= 32, cin * KK == KMAX, u8 frames.
#pragma once

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
#endif
  RB_FSTAMP(fst, 48);
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
    RB_FSTAMP(fst, img == img0 ? 57 : 58);
    commit();
    RB_FSTAMP(fst, img == img0 ? 59 : 60);
    __syncthreads();            // image complete (first image: weights and tap table as well)
    RB_FSTAMP(fst, img == img0 ? 49 : img == img0 + 1 ? 53 : 61);
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
    RB_FSTAMP(fst, img == img0 ? 50 : 54);
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
    RB_FSTAMP(fst, img == img0 ? 51 : 55);
    __syncthreads();            // every wave is done reading this image before the next one is committed
    if constexpr (TAIL16) {
      // the tail tile: reduction half 0 + half 1 (fixed order), bias, ReLU — waves 4 and 5, one channel half each.  The scratch
      // is written again only behind the next image's commit barrier.
      if (wave == 4 || wave == 5) {
        const int p = (NTILES - 1) * 32 + tx;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = tct * 16 + 4 * tkq + r;
          const float v = rb_t16_half_sum(s_tail, tu, r, lane);
          if (m < a.cout && p < G::P) outi[m * G::P + p] = fmaxf(v + tbias[r], 0.0f);
        }
      }
    }
    RB_FSTAMP(fst, img == img0 ? 52 : 56);
  }
}
