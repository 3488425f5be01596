// replay_search.h — the sum-tree search: SegmentTree._retrieve one value at a time (k_find) and the sampler's latency-optimised
// forms of it (LDS top + several levels per memory round trip).  Included by replay.hip only.
#pragma once
#include "replay_internal.h"

// ------------------------------------------------------------------------ find --
// SegmentTree._retrieve (memory.py:64-76) for ONE value: float64 value vs float32 nodes,
// strict '>' to go right, float64 subtraction, children clamped on the last internal
// level (memory.py:70-71).  Exactly L steps from the root.
__device__ __forceinline__ int64_t rb_tree_descend(const float* tree, int32_t levels, int64_t tree_start,
                                                   int64_t tree_len, double value) {
  int64_t node = 0;
  for (int32_t lv = 0; lv < levels; ++lv) {
    int64_t left = 2 * node + 1;
    int64_t right = left + 1;
    if (left >= tree_start) {  // children are leaves: bound outliers (memory.py:70-71)
      if (left > tree_len - 1) left = tree_len - 1;
      if (right > tree_len - 1) right = tree_len - 1;
    }
    const float lv_f = tree[left];
    const double lv_d = (double)lv_f;
    const bool go_right = value > lv_d;            // memory.py:73
    node = go_right ? right : left;                // memory.py:74
    if (go_right) value = __dsub_rn(value, lv_d);  // memory.py:75
  }
  return node;
}

__global__ __launch_bounds__(256) void k_find(ReplayView v, const double* values, int32_t n, float* probs,
                                               int64_t* data_idx, int64_t* tree_idx) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const int64_t leaf = rb_tree_descend(v.tree, v.levels, v.tree_start, v.tree_len, values[i]);
  probs[i] = v.tree[leaf];
  data_idx[i] = leaf - v.tree_start;
  tree_idx[i] = leaf;
}

// ---------------------------------------------------------------------- sample --
// Latency-optimised search used by the sampler: identical arithmetic to rb_tree_descend, but
//  (a) the top of the tree (<= 4095 nodes = 16 KB, levels 0..11) is staged once in LDS, and
//  (b) below that, up to five levels are fetched per memory round trip: the descendants of node u at
//      depth j are the 2^j consecutive entries starting at (u+1)*2^j - 1, so 2+4+8+16+32 independent
//      loads replace five dependent ones.  For the 1M-leaf tree: 11 LDS steps + 2 round trips
//      instead of 20 dependent HBM/L2 loads.
// Every load index is clamped to tree_len-1, which IS memory.py:70-71 on the leaf level and a
// no-op above it.
#define RB_TOP_NODES 4095    // levels 0..11 = 16 KB of LDS (16383 nodes = one round trip fewer measured SLOWER: 17.3 vs 15.7 us;
                             // fetching each sample's whole remaining subtree cooperatively into LDS, one trip: 26.9 us)

// D levels of the search with ONE batch of loads.  c holds level j (1..D) at [2^j - 2, 2^(j+1) - 2); `sel` is the path
// taken so far inside the fetched subtree (bit per level).  Register arrays are indexed through select chains only.
// (node indices are 32-bit here: capacity <= 2^30 keeps tree_len below 2^31, and 62 loads with 64-bit address arithmetic
// made a trip instruction-bound — ~1.8 us per trip against ~0.5 us of memory latency)
#define RB_TREE_PAD 64       // floats behind the last node that the search's 16-byte loads may touch (never used as values)
struct rb_f2u { float x, y; };                       // (plain structs: 4-byte alignment, filled with __builtin_memcpy)
struct rb_f4u { float x, y, z, w; };
template <int D>
__device__ __forceinline__ void rb_descend_levels(const float* tree, int32_t& node, double& value, int32_t last, float& nv) {
  float c[(2 << D) - 2];
  // level j = 2^j CONSECUTIVE entries from (node + 1) 2^j - 1 (an odd offset: dword-aligned only), loaded as unaligned 16-byte
  // vectors — 16 load instructions for five levels instead of 62: a wave's 64 samples touch 64 different lines per instruction, so
  // at batch 256 the address unit, not the latency, set the length of a trip (15 us per trip beside the optimiser stream, 6.6 at
  // batch 32).  An entry beyond the last node reads as tree[last] (the clamp above); the vectors themselves start at
  // min(base, last) and may run up to 2^D - 1 entries past the end: the tree buffer is padded for that (RB_TREE_PAD).
  const float t_last = tree[last];
#pragma unroll
  for (int j = 1; j <= D; ++j) {
    const uint32_t base = (((uint32_t)node + 1u) << j) - 1u;
    const float* src = tree + (base > (uint32_t)last ? (uint32_t)last : base);
    if (j == 1) {
      rb_f2u v;
      __builtin_memcpy(&v, src, 8);
      c[0] = base > (uint32_t)last ? t_last : v.x;
      c[1] = base + 1u > (uint32_t)last ? t_last : v.y;
    } else {
#pragma unroll
      for (int t = 0; t < (1 << j); t += 4) {
        rb_f4u v;
        __builtin_memcpy(&v, src + t, 16);
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) c[(1 << j) - 2 + t + u] = base + (uint32_t)(t + u) > (uint32_t)last ? t_last : e[u];
      }
    }
  }
  int sel = 0;
#pragma unroll
  for (int j = 1; j <= D; ++j) {
    float lf = c[(1 << j) - 2];                       // left child of the current path node: entry 2*sel of level j
#pragma unroll
    for (int t = 1; t < (1 << (j - 1)); ++t) lf = sel == t ? c[(1 << j) - 2 + 2 * t] : lf;
    const double l = (double)lf;
    const bool r = value > l;
    if (r) value = __dsub_rn(value, l);
    const uint32_t nx = 2u * (uint32_t)node + 1u + (r ? 1u : 0u);
    node = (int32_t)(nx > (uint32_t)last ? (uint32_t)last : nx);
    sel = 2 * sel + (r ? 1 : 0);
    if (j == D) {
      nv = c[(1 << j) - 2];
#pragma unroll
      for (int t = 1; t < (1 << j); ++t) nv = sel == t ? c[(1 << j) - 2 + t] : nv;
    }
  }
}

__device__ __forceinline__ int64_t rb_tree_descend_fast(const float* tree, const float* s_top, int n_cached,
                                                        int32_t levels, int64_t tree_len, double value,
                                                        float* node_value) {
  int32_t node = 0;
  int32_t lv = 0;
  float nv = 0.0f;                                  // tree[node] of the node reached (saves the caller a round trip)
  bool have_nv = false;
  const int32_t last = (int32_t)(tree_len - 1);
  for (; lv < levels; ++lv) {                       // LDS phase
    int32_t left = 2 * node + 1, right = left + 1;
    if (left > last) left = last;
    if (right > last) right = last;
    if (right >= n_cached) break;
    const double lv_d = (double)s_top[left];
    const bool go_right = value > lv_d;
    node = go_right ? right : left;
    if (go_right) value = __dsub_rn(value, lv_d);
    nv = s_top[node];
    have_nv = true;
  }
  // global phase: D levels per memory round trip (all 2^(D+1)-2 descendants of the current node are requested at once,
  // level j being the 2^j consecutive entries from (node+1)*2^j - 1), 5 while at least 5 remain: the 9 levels under the
  // LDS top of the 1M-leaf tree take two trips (5 + 4)
  while (lv < levels) {
    const int32_t rem = levels - lv;
    if (rem >= 5) { rb_descend_levels<5>(tree, node, value, last, nv); lv += 5; }
    else if (rem == 4) { rb_descend_levels<4>(tree, node, value, last, nv); lv += 4; }
    else if (rem == 3) { rb_descend_levels<3>(tree, node, value, last, nv); lv += 3; }
    else if (rem == 2) { rb_descend_levels<2>(tree, node, value, last, nv); lv += 2; }
    else { rb_descend_levels<1>(tree, node, value, last, nv); lv += 1; }
    have_nv = true;
  }
  // a child index clamped to the last node may not be the entry that was loaded for the unclamped slot: re-read then
  if (!have_nv || node == last) nv = tree[node];   // rare: explicit branch so the common path carries no load
  *node_value = nv;
  return (int64_t)node;
}

// The same search WITHOUT the LDS top: every level comes from global memory, up to six levels per round trip, the trips
// balanced (20 levels = 5+5+5+5, 17 = 6+6+5).  The nodes of the first trips are the same few KB for every sample and every
// launch (L2-resident, wave-wide broadcast loads); only the last trip reaches rows of the tree that miss.  Measured
// against the LDS-top variant (stage 16 KB, 11 LDS steps, 2 trips): see DESIGN.md §3 sampler row.
template <int DMAX>   // most levels per trip: 6 needs 126 registers for the fetched subtree (the <= 256-thread kernel only)
__device__ __forceinline__ int64_t rb_tree_descend_global(const float* tree, int32_t levels, int64_t tree_len, double value,
                                                          float* node_value) {
  int32_t node = 0;
  int32_t lv = 0;
  float nv = 0.0f;
  const int32_t last = (int32_t)(tree_len - 1);
  while (lv < levels) {
    const int32_t rem = levels - lv;
    const int32_t trips = (rem + DMAX - 1) / DMAX;
    const int32_t d = (rem + trips - 1) / trips;
    switch (d) {
      case 6: if (DMAX >= 6) { rb_descend_levels<(DMAX >= 6 ? 6 : 5)>(tree, node, value, last, nv); break; }
      case 5: rb_descend_levels<5>(tree, node, value, last, nv); break;
      case 4: rb_descend_levels<4>(tree, node, value, last, nv); break;
      case 3: rb_descend_levels<3>(tree, node, value, last, nv); break;
      case 2: rb_descend_levels<2>(tree, node, value, last, nv); break;
      default: rb_descend_levels<1>(tree, node, value, last, nv); break;
    }
    lv += d;
  }
  if (levels == 0 || node == last) nv = tree[node];
  *node_value = nv;
  return (int64_t)node;
}

// The first n_cached nodes of the tree into s_top, by the whole workgroup (rb_sample_main; k_update_sample, which stages before its
// write-back and keeps the copy current)
__device__ __forceinline__ void rb_stage_top(float* s_top, const float* tree, int n_cached) {
  for (int t = 4 * (int)threadIdx.x; t < n_cached; t += 4 * (int)blockDim.x) {   // 16-byte loads (the tree buffer is 16-byte aligned)
    if (t + 3 < n_cached) {
      *reinterpret_cast<float4*>(&s_top[t]) = *reinterpret_cast<const float4*>(&tree[t]);
    } else {
      for (int u = t; u < n_cached; ++u) s_top[u] = tree[u];
    }
  }
}
