// replay_append.h — the append kernels: one transition, one round of S streams (host or device operands), a bulk copy with its
// ancestor rebuild.  Included by replay.hip only.
#pragma once
#include "replay_internal.h"

// ---------------------------------------------------------------------- append --
// One transition (memory.py:105-108 + 56-61).  One 256-thread workgroup: quantise and
// store the frame with 4-byte packed writes, thread 0 walks the L sums to the root.
__global__ __launch_bounds__(256) void k_append_one(ReplayView v, const float* last_frame, int32_t timestep,
                                                     int32_t action, float reward, int32_t nonterminal) {
  const int64_t idx = v.hdr->index;
  const float prio = v.hdr->max;
  __syncthreads();  // every thread has read the header before thread 0 rewrites it
  uint32_t* dst = (uint32_t*)(v.frames + idx * RB_FRAME_BYTES);
  for (int w = (int)threadIdx.x; w < RB_FRAME_BYTES / 4; w += (int)blockDim.x) {
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // state[-1].mul(255).to(uint8): f32 multiply, truncating conversion (memory.py:106)
      const float x = __fmul_rn(last_frame[4 * w + j], 255.0f);
      const uint32_t q = (uint32_t)(int32_t)x & 0xFFu;
      packed |= q << (8 * j);
    }
    dst[w] = packed;
  }
  if (threadIdx.x == 0) {
    v.timestep[idx] = timestep;
    v.action[idx] = action;
    v.reward[idx] = reward;
    v.nonterminal[idx] = nonterminal ? 1 : 0;
    int64_t node = idx + v.tree_start;
    v.tree[node] = prio;  // memory.py:52
    while (node != 0) {   // memory.py:36-41
      const int64_t parent = (node - 1) / 2;
      v.tree[parent] = __fadd_rn(v.tree[2 * parent + 1], v.tree[2 * parent + 2]);
      node = parent;
    }
    const int64_t next = (idx + 1) % v.capacity;
    v.hdr->index = next;                 // memory.py:59
    if (next == 0) v.hdr->full = 1;      // memory.py:60
    v.hdr->total = v.tree[0];
    // memory.py:54,61: max(value, max) with value == max — unchanged
  }
}

// ---------------------------------------------------------------- append round --
// S interleaved environment streams (rb_replay_append_streams): one ROUND appends one transition per stream, stream s into
// ring slot start + s (start = the write head, a multiple of S: a round never wraps).  The same ring, tree and header as S
// calls of k_append_one in stream order: every leaf gets the running max (an append never changes it, memory.py:54,61) and
// every ancestor ends as fl32(left + right) of its final children, which is what the sequential walks leave behind.
// Blocks [0, S) quantise state[s][h-1] of stream s (f32 x 255, truncation: k_append_one's arithmetic) with 16-byte lanes;
// block S writes the columns and the leaves and rebuilds the ancestors.  The leaves of a round are CONTIGUOUS, so on every
// level the touched nodes form one range, and the only untouched nodes a level reads are the outside siblings at its two
// ends: block S requests all of them in one batch of loads, then walks the L levels in LDS (one barrier per level) — one
// round trip to memory instead of L dependent ones.  Per-stream scalars come by value in the argument block (AppendRound: host
// operands, no staging) or from device arrays (AppendRoundDev: rb_replay_append_streams_dev, a round whose operands never
// left the device); the kernel body is the same for both.  With device operands the timestep vector is in/out: the lane that
// stored stream t's timestep writes back the stream's next one (memory.py:108), so the caller keeps no host copy of it.
struct AppendRound {
  int32_t timestep[RB_MAX_STREAMS];
  int32_t action[RB_MAX_STREAMS];
  float reward[RB_MAX_STREAMS];
  uint8_t nonterminal[RB_MAX_STREAMS];
  static constexpr bool kDevice = false;
};
struct AppendRoundDev {
  int32_t* timestep;
  const int32_t* action;
  const float* reward;
  const uint8_t* nonterminal;
  static constexpr bool kDevice = true;
};
__device__ __forceinline__ uint32_t rb_quant4(float4 f) {
  // state[-1].mul(255).to(uint8) (memory.py:106), byte by byte as k_append_one
  const uint32_t q0 = (uint32_t)(int32_t)__fmul_rn(f.x, 255.0f) & 0xFFu;
  const uint32_t q1 = (uint32_t)(int32_t)__fmul_rn(f.y, 255.0f) & 0xFFu;
  const uint32_t q2 = (uint32_t)(int32_t)__fmul_rn(f.z, 255.0f) & 0xFFu;
  const uint32_t q3 = (uint32_t)(int32_t)__fmul_rn(f.w, 255.0f) & 0xFFu;
  return q0 | (q1 << 8) | (q2 << 16) | (q3 << 24);
}
template <class Ops>
__global__ __launch_bounds__(256) void k_append_streams(ReplayView v, const float* states, int64_t start, Ops a) {
  const int S = v.streams;
  const int t = (int)threadIdx.x;
  if ((int)blockIdx.x < S) {
    const int s = (int)blockIdx.x;
    const float4* src = (const float4*)(states + ((int64_t)s * v.history + (v.history - 1)) * RB_FRAME_BYTES);
    uint4* dst = (uint4*)(v.frames + (start + s) * RB_FRAME_BYTES);
    for (int w = t; w < RB_FRAME_BYTES / 16; w += (int)blockDim.x) {
      const float4 f0 = src[4 * w], f1 = src[4 * w + 1], f2 = src[4 * w + 2], f3 = src[4 * w + 3];
      dst[w] = make_uint4(rb_quant4(f0), rb_quant4(f1), rb_quant4(f2), rb_quant4(f3));
    }
    return;
  }
  __shared__ float s_val[2][RB_MAX_STREAMS + 2];     // values of the touched range of the current / next level
  __shared__ float s_out[RB_MAX_LEVELS][2];          // per level: the untouched sibling left of the range, right of it
  const int L = v.levels;
  const int64_t leaf0 = v.tree_start + start;
  if (t < S) {
    const int64_t idx = start + t;
    const int32_t ts = a.timestep[t];
    const uint8_t nt = a.nonterminal[t] ? 1 : 0;
    v.timestep[idx] = ts;                             // memory.py:107 (the stream's own episode timestep)
    v.action[idx] = a.action[t];
    v.reward[idx] = a.reward[t];
    v.nonterminal[idx] = nt;
    if constexpr (Ops::kDevice) a.timestep[t] = nt ? ts + 1 : 0;   // memory.py:108, per stream
    const float prio = v.hdr->max;                    // memory.py:107
    v.tree[leaf0 + t] = prio;
    s_val[0][t] = prio;
  } else if (t >= 64 && t < 64 + L) {                 // one lane per level: that level's outside siblings (one batch of loads)
    const int lv = t - 64;
    int64_t lo = leaf0, hi = leaf0 + S - 1;
    for (int k = 0; k < lv; ++k) { lo = (lo - 1) / 2; hi = (hi - 1) / 2; }
    s_out[lv][0] = (lo & 1) ? 0.0f : v.tree[lo - 1];  // lo a right child (even): its left sibling is outside the range
    s_out[lv][1] = (hi & 1) ? v.tree[hi + 1] : 0.0f;  // hi a left child (odd): its right sibling is outside
  }
  __syncthreads();
  int64_t lo = leaf0, hi = leaf0 + S - 1;
  int cur = 0;
  for (int lv = 0; lv < L; ++lv) {                   // memory.py:36-41 for every touched parent, bottom-up
    const int64_t plo = (lo - 1) / 2, phi = (hi - 1) / 2;
    if (t <= (int)(phi - plo)) {
      const int64_t p = plo + t;
      const int64_t l = 2 * p + 1, r = l + 1;
      const float lvv = l < lo ? s_out[lv][0] : s_val[cur][l - lo];
      const float rvv = r > hi ? s_out[lv][1] : s_val[cur][r - lo];
      const float x = __fadd_rn(lvv, rvv);           // memory.py:25
      s_val[cur ^ 1][t] = x;
      v.tree[p] = x;
    }
    __syncthreads();
    lo = plo; hi = phi; cur ^= 1;
  }
  if (t == 0) {
    const int64_t next = start + S == v.capacity ? 0 : start + S;
    v.hdr->index = next;                              // memory.py:59
    if (next == 0) v.hdr->full = 1;                   // memory.py:60
    v.hdr->total = s_val[cur][0];                     // the root
  }
}

// Bulk append: frames + columns + leaves (any grid), then ancestor rebuild kernels.
__global__ __launch_bounds__(256) void k_append_copy(ReplayView v, int64_t start, const uint8_t* frames,
                                                      const int32_t* timesteps, const int32_t* actions,
                                                      const float* rewards, const uint8_t* nonterminals, int64_t n) {
  constexpr int VEC = RB_FRAME_BYTES / 16;  // 441 uint4 per frame
  const float prio = v.hdr->max;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const int64_t idx = (start + i) % v.capacity;
    const uint4* s = (const uint4*)(frames + i * RB_FRAME_BYTES);
    uint4* d = (uint4*)(v.frames + idx * RB_FRAME_BYTES);
    for (int t = (int)threadIdx.x; t < VEC; t += (int)blockDim.x) d[t] = s[t];
    if (threadIdx.x == 0) {
      v.timestep[idx] = timesteps[i];
      v.action[idx] = actions[i];
      v.reward[idx] = rewards[i];
      v.nonterminal[idx] = nonterminals[i] ? 1 : 0;
      v.tree[idx + v.tree_start] = prio;
    }
  }
}

// tree[p] = tree[2p+1] + tree[2p+2] for p in [lo0,hi0] U [lo1,hi1] (inclusive; empty if hi<lo)
__global__ __launch_bounds__(256) void k_rebuild_ranges(float* tree, int64_t lo0, int64_t hi0, int64_t lo1, int64_t hi1) {
  const int64_t n0 = hi0 >= lo0 ? hi0 - lo0 + 1 : 0;
  const int64_t n1 = hi1 >= lo1 ? hi1 - lo1 + 1 : 0;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n0 + n1; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = t < n0 ? lo0 + t : lo1 + (t - n0);
    tree[p] = __fadd_rn(tree[2 * p + 1], tree[2 * p + 2]);
  }
}

// Finishes the rebuild from small ranges up to the root inside one workgroup, then
// publishes the new header.  ranges are NODE ranges at the level to process first.
__global__ __launch_bounds__(1024) void k_rebuild_top(ReplayView v, int64_t lo0, int64_t hi0, int64_t lo1, int64_t hi1,
                                                       int32_t have_ranges, int64_t new_index, int32_t set_full) {
  if (have_ranges) {
    for (;;) {
      const int64_t n0 = hi0 >= lo0 ? hi0 - lo0 + 1 : 0;
      const int64_t n1 = hi1 >= lo1 ? hi1 - lo1 + 1 : 0;
      for (int64_t t = threadIdx.x; t < n0 + n1; t += blockDim.x) {
        const int64_t p = t < n0 ? lo0 + t : lo1 + (t - n0);
        v.tree[p] = __fadd_rn(v.tree[2 * p + 1], v.tree[2 * p + 2]);
      }
      __threadfence_block();
      __syncthreads();
      if (lo0 == 0 || (n0 == 0 && lo1 == 0)) break;  // root done
      if (n0 > 0) { lo0 = (lo0 - 1) / 2; hi0 = (hi0 - 1) / 2; }
      if (n1 > 0) { lo1 = (lo1 - 1) / 2; hi1 = (hi1 - 1) / 2; }
      // merged / overlapping ranges only recompute the same node twice with the same value
    }
  }
  if (threadIdx.x == 0) {
    v.hdr->index = new_index;
    if (set_full) v.hdr->full = 1;
    v.hdr->total = v.tree[0];
  }
}
