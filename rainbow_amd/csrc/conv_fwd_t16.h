// conv_fwd_t16.h — the pieces of a whole-K 16x16x4 output tile that more than one forward kernel uses (rb_conv_fwd_body's T16 section
// and its half-units, k_conv_fwd_multi_t16, the tail units of k_conv_fwd_full): the lane's view of its tile, the bias fetch, the
// epilogue, and the sum of two reduction halves that met through LDS.  A section of conv_fwd.h.
#pragma once

// lane (x = l & 15, kq = l >> 4) of the wave that owns position tile pt and channel tile ct0 of a workgroup at position p0
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
// the epilogue of lane L's tile, whose channels start at mt: D[r] is channel mt + 4 kq + r at position L.p; relu(v + bias) goes to
// memory where the lane holds a position and the channel exists
template <class G>
__device__ __forceinline__ void rb_t16_store(const ConvLdsFwdArgs& a, int img, int mt, const ConvT16Lane& L, const rb_f32x4& v, const float (&b)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = mt + 4 * L.kq + r;
    if (L.pv && m < a.cout) rb_conv_store_out<G>(a, img, m, L.p, fmaxf(v[r] + b[r], 0.0f));
  }
}

// ---- two reduction halves of one tile on two waves: they meet through a scratch of [unit][4][64] floats -------------------------
// Four units: unit tu < 2 is the first reduction half of a tile, unit tu + 2 the second half of the same tile.  Every unit parks
// row r of its accumulator at s[(tu * 4 + r) * 64 + lane]; behind a barrier the first half's wave takes the sums.
// CONTRACT: row r of the tile is (half 0 + half 1) in that order, and the caller finishes it as (sum + bias), then ReLU (as
// rb_t16_store does): the order of these sums is what makes the split tile's output a fixed function of its inputs
__device__ __forceinline__ float rb_t16_half_sum(const float* s, int tu, int r, int lane) {
  return s[(tu * 4 + r) * 64 + lane] + s[((tu + 2) * 4 + r) * 64 + lane];
}
