// replay_stats.h — k_priority_stats: the shape of a replay's priority distribution (rb_replay_priority_stats) in one streamed
// pass over the leaves of the sum tree.  Included by replay.hip only.
//
// Workgroup g owns leaves [g * chunk, (g + 1) * chunk) — a partition fixed by the capacity alone — and leaves its double sums,
// its extremes and its counts in the handle's scratch; the histogram is built in LDS and added to the scratch's with integer
// atomics (exact in any order).  The last workgroup to arrive (stats_common.h) adds the doubles in a fixed order (chunks four per
// lane in chunk order, then a butterfly over the lanes), takes the integer
// totals out of the scratch with exchanges that put them back to zero, and overwrites the caller's struct: the same bits on
// every run.
#pragma once
#include "replay_internal.h"
#include "stats_common.h"

#define RB_PSTATS_THREADS 256
#define RB_PSTATS_MAX_WG 256      // at most this many chunks: the last workgroup folds their partials out of LDS, one per thread
#define RB_PSTATS_MIN_CHUNK 4096  // leaves per workgroup (16 per thread) until the capacity needs more than RB_PSTATS_MAX_WG of them
#define RB_PSTATS_LO_EXP (-40)    // floor(log2 p) of histogram bin 0
static_assert(sizeof(rb_priority_stats_t) == 296, "rb_priority_stats_t: two int64, two doubles, two floats, 64 int32");

struct PriorityScratch {
  double sum[RB_PSTATS_MAX_WG], sumsq[RB_PSTATS_MAX_WG];
  float max[RB_PSTATS_MAX_WG], min_pos[RB_PSTATS_MAX_WG];      // min_pos: +inf for a chunk without a valid non-zero leaf
  unsigned long long nonzero, invalid;                         // zero between launches, like hist and ticket
  int hist[64];
  unsigned ticket;
  unsigned pad;
};

struct PriorityStatsArgs {
  const float* leaves;            // [capacity]
  int64_t capacity, chunk;
  PriorityScratch* scratch;
  rb_priority_stats_t* out;
};

__global__ __launch_bounds__(RB_PSTATS_THREADS) void k_priority_stats(PriorityStatsArgs a) {
  __shared__ int s_hist[64];
  __shared__ double s_sum[RB_PSTATS_MAX_WG], s_sq[RB_PSTATS_MAX_WG];
  __shared__ float s_mx[RB_PSTATS_MAX_WG], s_mn[RB_PSTATS_MAX_WG];
  __shared__ unsigned long long s_cnt[2];
  __shared__ int s_flag;
  const int t = (int)threadIdx.x, lane = rb_lane(), wave = rb_wave();
  constexpr int NW = RB_PSTATS_THREADS / 64;
  if (t < 64) s_hist[t] = 0;
  if (t < 2) s_cnt[t] = 0ull;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * a.chunk;
  const int64_t hi = lo + a.chunk < a.capacity ? lo + a.chunk : a.capacity;
  double sum = 0.0, sq = 0.0;
  float mx = 0.0f, mn = INFINITY;
  unsigned long long nz = 0ull, bad = 0ull;
  for (int64_t i0 = lo + t; i0 < hi; i0 += 4 * RB_PSTATS_THREADS) {
    float p[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {                                   // four loads in flight; a leaf behind the chunk reads as an empty slot
      const int64_t i = i0 + u * RB_PSTATS_THREADS;
      p[u] = i < hi ? a.leaves[i] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned bits = __builtin_bit_cast(unsigned, p[u]);
      const unsigned e = (bits >> 23) & 0xffu;
      if (e == 0xffu || p[u] < 0.0f) { ++bad; continue; }           // NaN, inf (either sign), negative
      if (!(p[u] > 0.0f)) continue;                                 // zero (either sign): an empty slot
      ++nz;
      sum += (double)p[u]; sq += (double)p[u] * (double)p[u];
      mx = fmaxf(mx, p[u]); mn = fminf(mn, p[u]);
      int k = e == 0u ? 0 : (int)e - 127 - RB_PSTATS_LO_EXP;        // floor(log2 p) from the exponent field; denormals: bin 0
      k = k < 0 ? 0 : (k > 63 ? 63 : k);
      atomicAdd(&s_hist[k], 1);
    }
  }
  // ---- the workgroup's totals: waves in lane order (a fixed butterfly), then the waves in index order
  sum = rb_wave_sum_f64(sum); sq = rb_wave_sum_f64(sq);
  mx = rb_wave_max(mx); mn = -rb_wave_max(-mn);
  if (nz) atomicAdd(&s_cnt[0], nz);
  if (bad) atomicAdd(&s_cnt[1], bad);
  if (lane == 0) { s_sum[wave] = sum; s_sq[wave] = sq; s_mx[wave] = mx; s_mn[wave] = mn; }
  __syncthreads();
  PriorityScratch* sc = a.scratch;
  const int g = (int)blockIdx.x, G = (int)gridDim.x;
  if (t == 0) {
    double s = s_sum[0], q = s_sq[0];
    float m1 = s_mx[0], m0 = s_mn[0];
    for (int w = 1; w < NW; ++w) { s += s_sum[w]; q += s_sq[w]; m1 = fmaxf(m1, s_mx[w]); m0 = fminf(m0, s_mn[w]); }
    rb_pub_f64(sc->sum + g, s); rb_pub_f64(sc->sumsq + g, q);
    rb_pub_f32(sc->max + g, m1); rb_pub_f32(sc->min_pos + g, m0);
    if (s_cnt[0]) atomicAdd(&sc->nonzero, s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&sc->invalid, s_cnt[1]);
  }
  if (t < 64 && s_hist[t] != 0) atomicAdd(&sc->hist[t], s_hist[t]);
  if (!rb_last_arrival(&sc->ticket, (unsigned)G, &s_flag)) return;
  // ---- the fold (one workgroup)
  __syncthreads();                                                  // (s_sum .. s_mn are reused: thread 0 has read its waves' slots)
  if (t < G) { s_sum[t] = rb_sub_f64(sc->sum + t); s_sq[t] = rb_sub_f64(sc->sumsq + t); s_mx[t] = rb_sub_f32(sc->max + t); s_mn[t] = rb_sub_f32(sc->min_pos + t); }
  else { s_sum[t] = 0.0; s_sq[t] = 0.0; s_mx[t] = 0.0f; s_mn[t] = INFINITY; }      // (RB_PSTATS_MAX_WG == RB_PSTATS_THREADS slots)
  if (t < 64) a.out->hist[t] = atomicExch(&sc->hist[t], 0);
  __syncthreads();
  // the chunks' partials in chunk order, four per lane left to right, then the fixed butterfly over the lanes: wave 0 the sum, wave 1
  // the sum of squares, wave 2 the maximum, wave 3 the minimum (one thread walking 256 LDS words took ~16 us: profiles/diag_bench.txt)
  static_assert(RB_PSTATS_MAX_WG == RB_PSTATS_THREADS && NW == 4, "the fold reads four partials per lane, one quantity per wave");
  {
    const double* r = (wave == 0 ? s_sum : s_sq) + 4 * lane;
    const double tot = rb_wave_sum_f64(((r[0] + r[1]) + r[2]) + r[3]);
    const float* x = s_mx + 4 * lane;
    const float* n = s_mn + 4 * lane;
    const float fmx = rb_wave_max(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
    const float fmn = -rb_wave_max(-fminf(fminf(n[0], n[1]), fminf(n[2], n[3])));
    __syncthreads();
    if (lane == 0) {
      if (wave == 0) s_sum[0] = tot;
      if (wave == 1) s_sq[0] = tot;
      if (wave == 2) s_mx[0] = fmx;
      if (wave == 3) s_mn[0] = fmn;
    }
  }
  __syncthreads();
  if (t != 0) return;
  const double s = s_sum[0], q = s_sq[0];
  const float m1 = s_mx[0], m0 = s_mn[0];
  const unsigned long long nonzero = atomicExch(&sc->nonzero, 0ull), invalid = atomicExch(&sc->invalid, 0ull);
  a.out->nonzero = (int64_t)nonzero; a.out->invalid = (int64_t)invalid;
  a.out->sum = s; a.out->sumsq = q;
  a.out->max = m1; a.out->min_pos = nonzero ? m0 : 0.0f;
}
