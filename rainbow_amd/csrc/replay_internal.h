// replay_internal.h — pieces of the replay implementation shared inside librainbow_hip.so (not part of the C ABI):
// the kernel-side view of a replay handle, the sum-tree update bodies (replay_update.h), so the learner can run the priority
// write-back (agent.py:100) as one extra workgroup of its own backward launch instead of a separate dependent kernel, and the
// host interface of the early draw.  The only replay header another translation unit includes.
#pragma once
#include "rb_common.h"

struct ReplayView {
  int64_t capacity;
  int32_t history, n, levels;   // n: the EFFECTIVE horizon (rb_replay_set_horizon), 1 <= n <= the multi_step of creation.  The row
                        // stride of the window table, history + the multi_step of creation, is NOT in the view: any change of this
                        // struct's layout slowed the data-efficient step by ~1 us (profiles/horizon_bench.txt); the samplers read it
                        // from word RB_STRIDE_SLOT of the gamma^k table, the gathers take it as an argument
  int32_t streams;      // S interleaved environment streams (rb_replay_create_streams): stream s owns the slots s, s + S, s + 2S, ...
                        // (fills what was the padding in front of tree_start: the view keeps its size)
  int64_t tree_start, tree_len;
  float* tree;
  uint8_t* frames;
  int32_t* timestep;
  int32_t* action;
  float* reward;
  uint8_t* nonterminal;
  rb_replay_header_t* hdr;
  int32_t* dropped;     // pinned host word: write-backs dropped because their indices came from a failed draw (rb_replay_dropped_updates)
};

// floor_mod(a + d, m) for a in [0, m) and a SMALL offset d (window slots, write-head distance): conditional add /
// subtract instead of a 64-bit division (~100 instructions each; the sampler needs ~25 per sample).  The loops run
// at most once unless the ring is shorter than the window (degenerate capacities stay correct).
__device__ __forceinline__ int64_t rb_wrap(int64_t a, int64_t d, int64_t m) {
  int64_t x = a + d;
  while (x < 0) x += m;
  while (x >= m) x -= m;
  return x;
}
__device__ __forceinline__ int64_t rb_floor_mod(int64_t a, int64_t m) {
  int64_t r = a % m;
  return r < 0 ? r + m : r;
}

#define RB_STRIDE_SLOT 63     // word of the 64-word gamma^k table that holds the window table's row stride as an int32 (history + multi_step
                             // <= 64 and history >= 1, so gamma^63 is never needed)
#define RB_MAX_LEVELS 31     // deepest tree (capacity <= 2^30, rb_replay_create)

#include "replay_update.h"

// host side (replay.hip): kernel view + priority exponent of a handle
int rb_replay_internal_view(rb_replay_t* r, ReplayView* view, double* omega);

// ---- the early draw (host side: replay.hip; device side and the protocol: replay_spec.h; called by learner.hip train_step, not
// part of the C ABI)
struct rb_spec_request {
  const int64_t* upd_idx; const float* upd_loss; int32_t upd_n;     // the write-back (loss^w: rb_replay_update_priorities)
  int32_t batch; double priority_weight; int32_t max_attempts;      // the draw (rb_replay_sample with device RNG)
  int64_t* tree_idx; int64_t* actions; float* returns; float* nonterminals; float* weights;
  const unsigned* go_flag; unsigned go_epoch;                       // both kernels wait for *go_flag >= go_epoch first (NULL: no wait)
};
int rb_replay_spec_launch(rb_replay_t* r, const rb_spec_request& q);
// 0 once a cross-stream wait of an early pair has expired on this handle (until rb_replay_reset_failed_samples): the learner then
// keeps the write-back and the draw in its own launches
int rb_replay_spec_allowed(rb_replay_t* r);
// one shot: the NEXT draw on the handle may accept the tentative draw in flight (rb_learner_train_step only — it is the one caller
// that reads rb_replay_current_windows(); every public sample entry point redraws into table 0)
void rb_replay_spec_arm_accept(rb_replay_t* r);
int rb_replay_spec_inflight(rb_replay_t* r);
// the window table the LAST draw on the handle filled (rb_replay_buffers_t.window_dev is table 0; an accepted early draw used the other)
const int32_t* rb_replay_current_windows(rb_replay_t* r);
unsigned long long rb_replay_mutations(rb_replay_t* r);
// the effective horizon and discount of the handle (rb_replay_set_horizon), host values: what rb_learner_train_step compares with the
// learner's own before it draws
void rb_replay_horizon(rb_replay_t* r, int32_t* n_eff, double* discount);
