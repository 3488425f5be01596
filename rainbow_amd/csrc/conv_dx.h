// conv_dx.h — the input-gradient (transposed) convolution kernels: the weight operand they read (ConvWtJob, rb_conv_wt_block,
// rb_conv_wt16_block: written once per step by tenant workgroups of the head launch), the dY loader both kernels stage with
// (ConvDyLoader), k_conv_dx_lds (32x32x2 tiles, the reduction split over 8 waves) and k_conv_dx_t16_multi (whole-K 16x16x4 tiles, image
// loop).  Included by learner_internal.h.
#pragma once
#include "conv_stage.h"
#include "kernel_stamp.h"

// ---- the input-gradient kernels' weight operand, made once per step -------------------------------------------------------
// wT[phase][tile][k'][32]: element (co, c, ky, kx) of a layer's [cout][cin][KS][KS] weights goes to phase (ky % S, kx % S),
// channel tile c / 32, row k' = co * taps(phase) + (ky / S) * ntx(phase) + kx / S, column c % 32.  Runtime geometry (one
// body for every layer); `nblk` workgroups of any size share the elements.
struct ConvWtJob {
  const float* w;
  float* wT;
  int cin, cout, KS, S, kpad;
  int t16;                 // 1: the [phase][c][k'] layout of k_conv_dx_t16_multi (rb_conv_wt16_block), same buffer
};
// the [phase][c][k'] layout of k_conv_dx_t16_multi (wT16): k' = co * taps + ty * T + tx, every phase has the same T x T taps
__device__ __forceinline__ void rb_conv_wt16_block(const ConvWtJob& j, int blk, int nblk) {
  const int KK = j.KS * j.KS, total = j.cout * j.cin * KK, T = (j.KS + j.S - 1) / j.S, taps = T * T, kq = j.cout * taps;
  for (int e = blk * (int)blockDim.x + (int)threadIdx.x; e < total; e += nblk * (int)blockDim.x) {
    const int co = e / (j.cin * KK), r = e - co * (j.cin * KK);
    const int c = r / KK, tap = r - c * KK;
    const int ky = tap / j.KS, kx = tap - ky * j.KS;
    const int py = ky % j.S, px = kx % j.S, ty = ky / j.S, tx = kx / j.S;
    j.wT[((int64_t)(py * j.S + px) * j.cin + c) * kq + co * taps + ty * T + tx] = j.w[e];
  }
}
__device__ __forceinline__ void rb_conv_wt_block(const ConvWtJob& j, int blk, int nblk) {
  if (j.t16) { rb_conv_wt16_block(j, blk, nblk); return; }        // block-uniform
  const int KK = j.KS * j.KS, total = j.cout * j.cin * KK, ntiles = (j.cin + 31) / 32;
  for (int e = blk * (int)blockDim.x + (int)threadIdx.x; e < total; e += nblk * (int)blockDim.x) {
    const int co = e / (j.cin * KK), r = e - co * (j.cin * KK);
    const int c = r / KK, tap = r - c * KK;
    const int ky = tap / j.KS, kx = tap - ky * j.KS;
    const int py = ky % j.S, px = kx % j.S, ty = ky / j.S, tx = kx / j.S;
    const int nty = (j.KS - py + j.S - 1) / j.S, ntx = (j.KS - px + j.S - 1) / j.S;
    const int kp = co * (nty * ntx) + ty * ntx + tx;
    j.wT[(((int64_t)(py * j.S + px) * ntiles + (c >> 5)) * j.kpad + kp) * 32 + (c & 31)] = j.w[e];
  }
}

// ========================================================================= data gradient ==
// dX[img][c][y][x] = relu'(x_act) * sum_{co,ky,kx} W[co][c][ky][kx] * dY[img][co][(y-ky)/S][(x-kx)/S]
// decomposed by phase (y % S, x % S) so only real taps are visited.  The whole dY image sits in LDS.
// grid = (phases S*S * position groups of 32*NT, cin / 32, images B); block = 512.
struct ConvLdsDxArgs {
  int cin, cout;
  const float* w;        // [cout][cin][KS][KS]
  const float* wT;       // the same weights as the kernel wants them: [phase][32-channel tile][KPAD rows k' = (co, tap)][32]
                         // (rb_conv_wt_block below writes it earlier in the step, as tenant workgroups of the head launch)
  const float* dy;       // [B][cout][P]
  const float* x_act;    // [NI][cin][IP] (rows [0,B))
  float* dx;             // [B][cin][IP]
  // LAZY instantiation only (the last conv layer): dY is not materialised — the staging sums the hidden layer's
  // dy_splits (<= 4) row-split partials [s][B][cout * P] and applies relu'(dy_mask) itself
  const float* dy_part;
  const float* dy_mask;  // the layer's own activation, rows [0,B)
  int64_t dy_stride;     // floats between partials
  int dy_splits;
  int ipb, batch;        // MULTI instantiation: images per workgroup (grid z = ceil(batch / ipb)), image count
  int img_fast;          // grid = (image groups, channel tiles, phase x position groups): see ConvLdsFwdArgs::img_fast (conv_fwd.h)
};

// ---- dY of one image for both data-gradient kernels: global loads into registers (issue), LDS stores later (commit) ----------------
// Thread t of THREADS owns elements e = t + i * THREADS, i < LIT, of the [cout][P] image.
// The staging of these kernels is INSTRUCTION-bound, not memory-bound (fine-grained stamps, tools/stamp/fine_dx.py: 7.5 us from
// workgroup start to the first MFMA with every load landed at 3.3 us — two waves per SIMD executing ~2000 VALU
// instructions of index arithmetic each).  So: only the INTERIOR cells of dY are loaded and stored (contiguous in memory:
// no halo-indexed gather), the zero halo is one block of 16-byte stores at kernel start (rb_lds_zero), all offsets are 32-bit and
// go through buffer loads (no 64-bit pointer arithmetic per load).
// LAZY (the last conv layer): the mask and every partial of a thread's cells are requested before the first add (one round trip);
// commit forms dY = rb_dy_lazy(mask, partials) on the way into LDS.
template <int N, int THREADS>
__device__ __forceinline__ void rb_lds_zero(float* s, int t) {
  for (int e = t; e < N / 4; e += THREADS) rb_st4(s + 4 * e, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  for (int e = N / 4 * 4 + t; e < N; e += THREADS) s[e] = 0.0f;
}
template <class G, int THREADS, int LIT, bool LAZY>
struct ConvDyLoader {
  float pre_m[LAZY ? LIT : 1], pre_p[LAZY ? LIT : 1][4], pre_v[LAZY ? 1 : LIT];
  int cell[LIT];                                        // LDS cell of this thread's i-th interior element (image-independent), -1 = none
  // the LDS image: planes PP apart, rows PW apart, PAD halo cells in front of every row and plane
  template <int PP, int PW, int PAD>
  __device__ __forceinline__ void cells(int t, int ni) {
#pragma unroll
    for (int i = 0; i < LIT; ++i) {
      const int e = t + i * THREADS;
      const int ec = e < ni ? e : ni - 1;
      const int co = ec / G::P, r = ec - co * G::P;
      const int y = r / G::OH, x = r - y * G::OH;
      cell[i] = e < ni ? co * PP + (y + PAD) * PW + x + PAD : -1;
    }
  }
  __device__ __forceinline__ void issue(const ConvLdsDxArgs& a, int t, int ni, int img) {
    const unsigned ibase = 4u * (unsigned)(img * ni);
    if constexpr (LAZY) {
      const rb_buf mk = rb_make_buf(a.dy_mask);
      rb_buf pp[4];
#pragma unroll
      for (int sp = 0; sp < 4; ++sp) pp[sp] = rb_make_buf(a.dy_part + (int64_t)(sp < a.dy_splits ? sp : a.dy_splits - 1) * a.dy_stride);
#pragma unroll
      for (int i = 0; i < LIT; ++i) {
        const int e = t + i * THREADS;
        const unsigned off = 4u * (unsigned)(e < ni ? e : ni - 1);
        pre_m[i] = rb_ld1_buf(mk, off, ibase);
#pragma unroll
        for (int sp = 0; sp < 4; ++sp) pre_p[i][sp] = rb_ld1_buf(pp[sp], off, ibase);
      }
    } else {
      const rb_buf src = rb_make_buf(a.dy);
#pragma unroll
      for (int i = 0; i < LIT; ++i) {
        const int e = t + i * THREADS;
        pre_v[i] = rb_ld1_buf(src, 4u * (unsigned)(e < ni ? e : ni - 1), ibase);
      }
    }
  }
  __device__ __forceinline__ void commit(const ConvLdsDxArgs& a, float* s_dy) const {
#pragma unroll
    for (int i = 0; i < LIT; ++i)
      if (cell[i] >= 0) {
        if constexpr (LAZY) s_dy[cell[i]] = rb_dy_lazy(pre_m[i], pre_p[i], a.dy_splits);
        else s_dy[cell[i]] = pre_v[i];
      }
  }
};

// k_conv_dx_lds's weight slab [k' = (co, tap of this phase)][32 channels c0 ..], rows WLD apart: it arrives READY-MADE from a.wT —
// written once per step by tenant workgroups of the head launch (rb_conv_wt_block), rows >= K and channels >= cin zero — as
// 16-byte loads and 16-byte LDS stores.  Gathering it in the kernel from the [co][c][ky][kx] weights cost every workgroup
// 3.8-4.3 us of its 7.4-7.7 (tools/wg_timeline.py: ~2000 VALU instructions of index arithmetic per thread in front of the first
// MFMA).  (rb_slab_copy is the same idea for [32][K] slabs, one loop; here every load is issued before the first store.)
template <int KPAD, int WLD, int WK>
__device__ __forceinline__ void rb_dx_stage_slab(float* s_w, const float* src, int t, int wgi) {
  constexpr int NQ = (KPAD * 8 + RB_CONV_THREADS - 1) / RB_CONV_THREADS;     // float4s of the slab per thread
  (void)wgi;
  float4 v[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    int e = t + i * RB_CONV_THREADS;
    if (e > KPAD * 8 - 1) e = KPAD * 8 - 1;
    v[i] = rb_ld4(src + 4 * e);
  }
#if defined(RB_STAMP) && defined(RB_STAMP_FINE)
  RB_WGT(WK + 3, wgi, 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  RB_WGT(WK + 3, wgi, 2);
#endif
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int e = t + i * RB_CONV_THREADS;
    if (e < KPAD * 8) rb_st4(s_w + (e >> 3) * WLD + 4 * (e & 7), v[i]);
  }
}

// MULTI (batches of 64 and more, the data-efficient second layer; the canonical layers' image loop is k_conv_dx_t16_multi below):
// a workgroup keeps its weight slab and walks a.ipb images — per image only the dY tile is staged; the reduction scratch then
// has a region of its own instead of overlaying the operands.
template <class G, int NT, int COUT, bool LAZY = false, bool MULTI = false>
__global__ __launch_bounds__(RB_CONV_THREADS) void k_conv_dx_lds(ConvLdsDxArgs a) {
  constexpr int TMAX = (G::KS + G::S - 1) / G::S;           // taps per dimension of a phase
  constexpr int KMAX = COUT * TMAX * TMAX;
  constexpr int KPAD = (KMAX + 2 * RB_CONV_WAVES - 1) / (2 * RB_CONV_WAVES) * (2 * RB_CONV_WAVES);
  // dY sits in LDS with a zero halo: every (position, tap) pair then addresses a legal cell and the
  // MFMA loop needs no bounds tests (with them it ran at a quarter of the MFMA rate: 4.1 us for 1 us of MFMAs)
  // (low side: TMAX-1 taps reach before the first output; high side: phase positions up to ceil(IH/S)-1, which also
  // covers input rows no output touches when (OH-1)*S + KS < IH)
  constexpr int PAD = TMAX - 1, PADH = (G::IH + G::S - 1) / G::S - G::OH, PW = G::OH + PAD + PADH, PP = PW * PW;
  constexpr int RED = RB_CONV_WAVES * NT * 16 * 64;
  // row stride of the [k'][c] weight slab.  The MFMA operand read (32 consecutive c of a row) is conflict-free at any stride;
  // the stride-1 staging stores are not: a thread holds 4 consecutive elements of a (c, tap) run, lanes 4 elements apart, and
  // with 33 the bank is (tap + c) mod 32 — 8.8 lanes per bank on average (SQ_LDS_BANK_CONFLICT: 61 % of the kernel's LDS
  // cycles); 38 spreads them to 2.0 per bank
  constexpr int WLD = 36;      // (16-byte aligned rows: the slab is a straight copy of a.wT, 16-byte loads -> 16-byte LDS stores)
  constexpr int OPS = KPAD * WLD + COUT * PP;
  constexpr int WSZ = MULTI ? OPS + RED : (OPS > RED ? OPS : RED);
  __shared__ __attribute__((aligned(16))) float s_all[WSZ];
  float* s_w = s_all;
  float* s_dy = s_all + KPAD * WLD;
  float* s_red = MULTI ? s_all + OPS : s_all;
  __shared__ int s_koff[KPAD];      // co*PP - ty*PW - tx

  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  constexpr int WK = G::KS == 3 ? 3 : 4;                   // timeline ids (RB_STAMP builds only)
  const int wgi = (int)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z));
  (void)wgi;
  RB_WGT(WK, wgi, 0);
  RB_WGT_HW(WK, wgi);
  const int ipb = MULTI ? a.ipb : 1;
  const int bx_ = a.img_fast ? (int)blockIdx.z : (int)blockIdx.x, bz_ = a.img_fast ? (int)blockIdx.x : (int)blockIdx.z;
  const int img0 = bz_ * ipb;
  const int c0 = (int)blockIdx.y * 32;
  const int phase = bx_ % (G::S * G::S);
  const int n0 = (bx_ / (G::S * G::S)) * (32 * NT);                 // first position of this block inside the phase
  const int py = phase / G::S, px = phase % G::S;
  const int nty = (G::KS - py + G::S - 1) / G::S, ntx = (G::KS - px + G::S - 1) / G::S;
  const int nyy = (G::IH - py + G::S - 1) / G::S, nxx = (G::IH - px + G::S - 1) / G::S;
  const int taps = nty * ntx;
  const int K = a.cout * taps;
  const int npos = nyy * nxx;
  if (n0 >= npos) return;                                            // block-uniform

  // ---- once per workgroup: the tap table and the phase's weight slab transposed to [k'][c]
  for (int k = t; k < KPAD; k += RB_CONV_THREADS) {
    const int kc = k < K ? k : K - 1;
    const int co = kc / taps, r = kc - co * taps;
    const int ty = r / ntx, tx = r - ty * ntx;
    s_koff[k] = co * PP - ty * PW - tx;
  }
  constexpr int KW = KPAD / RB_CONV_WAVES;            // even, compile-time (rows >= K of s_w are zero): full unroll
  const int kb = wave * KW;
  int noff[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    int n = n0 + nt * 32 + (lane & 31);
    if (n > npos - 1) n = npos - 1;
    const int yy = n / nxx, xx = n - yy * nxx;
    noff[nt] = (yy + PAD) * PW + xx + PAD;
  }
  const int kh = lane >> 5, ml = lane & 31;
  // the epilogue's cells (they do not depend on the image): offset inside the image, -1 = nothing to store
  constexpr int EIT = (NT * 16 * 64) / RB_CONV_THREADS;
  int eoff[EIT];
#pragma unroll
  for (int it = 0; it < EIT; ++it) {
    const int idx = t + it * RB_CONV_THREADS;
    const int l = idx & 63, r = (idx >> 6) & 15, nt = idx >> 10;
    const int c = c0 + rb_mfma_row(r, l);
    const int n = n0 + nt * 32 + (l & 31);
    const int yy = n / nxx, xx = n - yy * nxx;
    eoff[it] = (c < a.cin && n < npos) ? c * G::IP + (yy * G::S + py) * G::IH + xx * G::S + px : -1;
  }
  int kos[KW / 2];                                    // tap offsets of this wave's k range, off the per-step critical path

  // dY of an image (ConvDyLoader): with MULTI the next image's loads are in flight under this image's MFMA loop and reduction
  constexpr int LIT = (COUT * G::P + RB_CONV_THREADS - 1) / RB_CONV_THREADS;
  ConvDyLoader<G, RB_CONV_THREADS, LIT, LAZY> dyl;
  const int ni = a.cout * G::P;
  dyl.template cells<PP, PW, PAD>(t, ni);
  if (PW > G::OH) rb_lds_zero<COUT * PP, RB_CONV_THREADS>(s_dy, t);   // the whole haloed image once: the halo stays zero from image to image

  dyl.issue(a, t, ni, img0);
#if defined(RB_STAMP) && defined(RB_STAMP_FINE)
  RB_WGT(WK + 3, wgi, 0);
#endif
  // (the weight slab is staged AFTER the first image's dY loads have been issued: its own loads then share their round
  // trip instead of preceding it)
  rb_dx_stage_slab<KPAD, WLD, WK>(s_w, a.wT + ((int64_t)(phase * ((a.cin + 31) / 32) + (int)blockIdx.y) * KPAD) * 32, t, wgi);

#if defined(RB_STAMP) && defined(RB_STAMP_FINE)
  RB_WGT(WK + 3, wgi, 3);
#endif
  if (PW > G::OH) __syncthreads();                    // the zero fill (other threads' cells) precedes the interior stores
  for (int ii = 0; ii < ipb; ++ii) {
    const int img = img0 + ii;
    if (MULTI && img >= a.batch) break;               // block-uniform
    dyl.commit(a, s_dy);
#if defined(RB_STAMP) && defined(RB_STAMP_FINE)
    if (ii == 0) RB_WGT(WK + 3, wgi, 4);
#endif
    // the ReLU mask of this image's output cells: requested now, consumed after the MFMA loop (in the epilogue the load
    // sat on the critical path of every store)
    const float* xa = a.x_act + (int64_t)img * a.cin * G::IP;
    float mask[EIT];
#pragma unroll
    for (int it = 0; it < EIT; ++it) mask[it] = xa[eoff[it] >= 0 ? eoff[it] : 0];
    __syncthreads();            // operands complete (and, MULTI, the previous image's reduction scratch has been consumed)
    if (ii == 0) { RB_WGT(WK, wgi, 1); RB_WGT(WK, wgi, 2); RB_WGT(WK, wgi, 3); }
    if (MULTI && ii + 1 < ipb && img + 1 < a.batch) dyl.issue(a, t, ni, img + 1);
    if (ii == 0) {
#pragma unroll
      for (int j = 0; j < KW / 2; ++j) kos[j] = s_koff[kb + 2 * j + kh];
    }
    rb_f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nt][r] = 0.0f;
#pragma unroll
    for (int j = 0; j < KW / 2; ++j) {
      const float av = s_w[(kb + 2 * j + kh) * WLD + ml];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = rb_mfma32(av, s_dy[kos[j] + noff[nt]], acc[nt]);
    }
    if (ii == 0) RB_WGT(WK, wgi, 4);
    if (!MULTI) __syncthreads();                      // the scratch overlays the operands
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) s_red[((wave * NT + nt) * 16 + r) * 64 + lane] = acc[nt][r];
    __syncthreads();                                  // (MULTI: every wave is also done reading this image's dY)
    float* dxi = a.dx + (int64_t)img * a.cin * G::IP;
#pragma unroll
    for (int it = 0; it < EIT; ++it) {
      const int idx = t + it * RB_CONV_THREADS;
      const int l = idx & 63, r = (idx >> 6) & 15, nt = idx >> 10;
      float v = s_red[((0 * NT + nt) * 16 + r) * 64 + l];
#pragma unroll
      for (int wv = 1; wv < RB_CONV_WAVES; ++wv) v += s_red[((wv * NT + nt) * 16 + r) * 64 + l];
      if (eoff[it] >= 0) {
        const float o = mask[it] > 0.0f ? v : 0.0f;
        dxi[eoff[it]] = o;
      }
    }
  }
  RB_WGT(WK, wgi, 5);
  RB_WGT(WK, wgi, 6);
}

// ---- the same data gradient on whole-K 16x16x4 tiles, for the image loop of large batches (round 6) -----------------------------
// k_conv_dx_lds<..., MULTI> splits the reduction over its 8 waves and sums the partial tiles through LDS for every image — the pattern
// k_conv_fwd_multi_t16 removed from the forward (MFMA-busy 0.38 / 0.46 at batch 256, half of the launch spent outside the MFMA loop).
// Here a workgroup owns (stride phase, 32 input channels, ALL positions of the phase): one wave per 16-position x 16-channel tile runs the
// WHOLE reduction k' = (co, tap) for its tile — lane (x, kq) takes the contiguous quarter [kq K'/4, (kq + 1) K'/4), its A operands are
// whole float4s of weight row c (the slab arrives ready-made as wT16[phase][c][k'], rb_conv_wt16_block), its B operands are cells of
// the zero-haloed dY image at compile-time offsets co PPL - ty PW - tx — and the epilogue (relu' mask, store) goes from the accumulators
// to memory.  Needs KS % S == 0 (every phase has the same taps), (COUT * taps) % 16 == 0, cin % 32 == 0 (host-checked).
// grid = (phases, cin / 32, image groups) or image-group-fastest (a.img_fast); block = 64 * NWV.
template <class G, int COUT>
struct ConvDxT16 {
  static constexpr int TMAX = (G::KS + G::S - 1) / G::S, TAPS = TMAX * TMAX;
  static constexpr int KP = COUT * TAPS, KQ = KP / 4, CQ = COUT / 4, WS = KP + 4;
  static constexpr int PAD = TMAX - 1, NS = (G::IH + G::S - 1) / G::S, PADH = NS - G::OH, PW = G::OH + PAD + PADH, PP = PW * PW;
  static constexpr int rb_pad() {
    for (int p = 0; p < 64; ++p)
      if ((CQ * (PP + p)) % 32 == 16) return p;
    return 0;
  }
  static constexpr int PPL = PP + rb_pad();                    // dY plane stride: the four k-quarters of an operand read start 16 banks apart
  // step j = (co, tap) of the reduction -> offset of its dY cell from the lane's position (rb_t16_steps)
  static __device__ __forceinline__ constexpr int at(int j) { return (j / TAPS) * PPL - ((j % TAPS) / TMAX) * PW - (j % TAPS) % TMAX; }
  static constexpr int NPOS = NS * NS, PT = (NPOS + 15) / 16, TILE_WAVES = 2 * PT, NWV = (TILE_WAVES + 3) / 4 * 4;
  static constexpr int FLOATS = 32 * WS + COUT * PPL;
  static constexpr bool OK = (G::KS % G::S) == 0 && (KP % 16) == 0 && (COUT % 4) == 0 && NWV <= 16 && FLOATS * 4 <= 150 * 1024;
};
template <class G, int COUT, bool LAZY>
__global__ __launch_bounds__((64 * ConvDxT16<G, COUT>::NWV)) void k_conv_dx_t16_multi(ConvLdsDxArgs a) {
  typedef ConvDxT16<G, COUT> Z;
  constexpr int THREADS = 64 * Z::NWV, WS = Z::WS, PPL = Z::PPL, PW = Z::PW, PAD = Z::PAD, KQ = Z::KQ, CQ = Z::CQ;
  static_assert(Z::OK, "k_conv_dx_t16_multi: geometry");
  __shared__ __attribute__((aligned(16))) float smem[Z::FLOATS];
  float* s_w = smem;
  float* s_dy = smem + 32 * WS;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int bx_ = a.img_fast ? (int)blockIdx.z : (int)blockIdx.x, bz_ = a.img_fast ? (int)blockIdx.x : (int)blockIdx.z;
  const int img0 = bz_ * a.ipb;
  const int img_end = img0 + a.ipb < a.batch ? img0 + a.ipb : a.batch;
  if (img0 >= a.batch) return;                                // block-uniform
  const int c0 = (int)blockIdx.y * 32;
  const int phase = bx_;
  const int py = phase / G::S, px = phase % G::S;
  const int nyy = (G::IH - py + G::S - 1) / G::S, nxx = (G::IH - px + G::S - 1) / G::S;
  const int npos = nyy * nxx;
  // ---- dY of an image: interior cells only, global loads into registers (issue), LDS stores later (commit); the zero halo is
  // written once (k_conv_dx_lds: the staging of these kernels is instruction-bound)
  constexpr int LIT = (COUT * G::P + THREADS - 1) / THREADS;
  ConvDyLoader<G, THREADS, LIT, LAZY> dyl;
  const int ni = a.cout * G::P;
  dyl.template cells<PPL, PW, PAD>(t, ni);
  rb_lds_zero<COUT * PPL, THREADS>(s_dy, t);
  dyl.issue(a, t, ni, img0);
  // the slab [32 channels c0 ..][K'] of this phase: a straight copy of a.wT (wT16 layout), rows of channels >= cin zero
  rb_slab_copy<Z::KP / 4, WS, THREADS>(s_w, a.wT + ((int64_t)phase * a.cin + c0) * Z::KP, Z::KP, a.cin - c0, t);
  // ---- this wave's tile: position tile pt, channel tile ct0; lane (x, kq)
  const bool tile_wave = wave < Z::TILE_WAVES;
  const int pt = wave % Z::PT, ct0 = (wave / Z::PT) % 2;
  const int x = lane & 15, kq = lane >> 4;
  int n = pt * 16 + x;
  const bool pv = n < npos;
  if (n > npos - 1) n = npos - 1;
  const int yy = n / nxx, xx = n - yy * nxx;
  const float* bp = s_dy + kq * CQ * PPL + (yy + PAD) * PW + xx + PAD;
  const float* ap = s_w + (ct0 * 16 + x) * WS + kq * KQ;
  int eoff[4];                                          // the lane's four output cells (channel 4 kq + r of its tile): offset in the image, -1 = none
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = c0 + ct0 * 16 + 4 * kq + r;
    eoff[r] = (pv && c < a.cin) ? c * G::IP + (yy * G::S + py) * G::IH + xx * G::S + px : -1;
  }
  __syncthreads();                                      // zero fill complete before the first interior stores (other threads' cells)
  for (int img = img0; img < img_end; ++img) {
    dyl.commit(a, s_dy);
    const float* xa = a.x_act + (int64_t)img * a.cin * G::IP;
    float mask[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) mask[r] = xa[eoff[r] >= 0 ? eoff[r] : 0];
    __syncthreads();                                    // dY (and the slab) complete
    if (img + 1 < img_end) dyl.issue(a, t, ni, img + 1);
    if (tile_wave) {
      rb_f32x4 acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = 0.0f;
      rb_t16_steps<Z, WS, 0, KQ / 4>(ap, bp, acc);
      float* dxi = a.dx + (int64_t)img * a.cin * G::IP;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (eoff[r] >= 0) dxi[eoff[r]] = mask[r] > 0.0f ? acc[r] : 0.0f;
    }
    __syncthreads();                                    // every wave is done reading this image's dY
  }
}
