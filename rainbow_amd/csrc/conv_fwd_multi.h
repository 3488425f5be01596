// conv_fwd_multi.h — large batches, later layers: k_conv_fwd_multi_t16, one weight slab per workgroup and a loop over images around
// the whole-K 16x16x4 tile.  A section of conv_fwd.h.
//
// At 768 images the one-image workgroup (conv_fwd_image.h) stages 34-76 KB of weights for 2.6-5.3 us of MFMAs, 6-15 times per CU.  Here a
// workgroup owns (position chunk, 32-channel slab) and walks a.ipb images.  The workgroup is the t16 body's
// (rb_conv_fwd_body<..., T16 = true>): one wave per 16-position x 16-channel tile over the WHOLE reduction, the epilogue straight from
// the accumulators — no partial sums, no reduction scratch (a split reduction idles the MFMA pipe during its per-image sums:
// MFMA-busy 0.53-0.57 at batch 256, profiles/round5_sq_counters_*), two barriers per image (patch complete / patch free).  The
// row-major 32-channel slab (and the bias terms) are set up once per net (again where the image range crosses from the online to
// the target net), the next image's patch is in flight (registers) under this image's MFMA loop.  Same LDS image as the one-image
// t16 kernel (117 / 95 KB for the canonical layers 2 / 3).  Needs cin * KK == KMAX, cin % 4 == 0, KMAX % 16 == 0, cout % 32 == 0
// (true of every later layer of the canonical stack).
// grid = (position chunks, cout / 32, image groups) or image-group-fastest (a.img_fast); block = 64 * NWV.
#pragma once

template <class G, int NT, int PR, int KMAX, int PCH = 32 * NT>
__global__ __launch_bounds__((64 * ConvFwdWaves<KMAX, PCH, true>::NWV))
void k_conv_fwd_multi_t16(ConvLdsFwdArgs a) {
  typedef ConvFwdLdsSize<G, PR, KMAX, true> SZ;
  typedef ConvFwdWaves<KMAX, PCH, true> WV;
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
  // ---- the patch of one image: loads into registers (issue), de-interleaved LDS stores later (commit)
  constexpr bool x_vec = (G::IH % 4) == 0;
  constexpr int XV = x_vec ? (CMAX * PR * G::IH / 4 + THREADS - 1) / THREADS : 1;
  constexpr int XS = x_vec ? 1 : (CMAX * PR * G::IH + THREADS - 1) / THREADS;
  const int v4 = per_c >> 2, total4 = cin * v4, total1 = cin * per_c;
  float4 xv[XV];
  float xs[XS];
  auto issue = [&](int img) {                         // (every load is issued, at a clamped index)
    const float* xbase = a.in_f + (int64_t)img * cin * G::IP;
    if constexpr (x_vec) rb_patch_issue<G, true, XV, THREADS>(xv, xbase, iy0 * G::IH, t, v4, total4);
    else rb_patch_issue<G, true, XS, THREADS>(xs, xbase, iy0 * G::IH, t, per_c, total1);
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
    rb_f32x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = 0.0f;
    rb_t16_steps<SZ, SZ::WS, 0, KQ / 4>(L.ap, bpi, acc);
    // (rb_t16_store's loop, written out: through the helper the third layer's instantiation allocates one more VGPR)
#pragma unroll
    for (int r = 0; r < 4; ++r) {                     // D[r]: channel 4 kq + r of the tile, position x
      const int m = cout0 + ct0 * 16 + 4 * L.kq + r;
      if (L.pv && m < a.cout) rb_conv_store_out<G>(a, img, m, L.p, fmaxf(acc[r] + bias4[r], 0.0f));
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
