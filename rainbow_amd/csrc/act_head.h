// act_head.h — the head of Agent.act / evaluate_q (agent.py:53-55, 110-112) for ONE logits row: the dueling combine, the expected
// value of every action's C51 distribution, the argmax, the optional e-greedy draw (agent.py:58-59) and the store of
// (action, q) a polling host may read.  One body, rb_head_act_body, for every caller.
// Included by act_path.h (k_act_fused runs it as its last phase) and by head.h (k_head_act, k_head_act_eps, k_act_eps_override);
// needs rb_common.h (rb_philox) and rb_device.h (the wave reductions).
#pragma once
#include "rb_common.h"
#include "rb_device.h"

// q = v + a - mean_a(a)          model.py:75
__device__ __forceinline__ float rb_dueling_q(const float* lg, const float* mean_a, int Z, int a, int z) {
  return (lg[z] + lg[Z + a * Z + z]) - mean_a[z];
}
// Agent.act / evaluate_q head (agent.py:53-55, 110-112) for ONE image: `lg` = its logits row (global or LDS), s_mean [Z]
// and s_ev [A] workgroup scratch.  All threads of a 256-thread workgroup call.  err (optional): the word an expired in-launch
// wait of launch number `err_epoch` sets to that number -> action -1 for THAT launch only (a later launch compares with its own
// number: the failure state needs no reset and cannot stick).
// epsilon >= 0 (rb_learner_act_batch_eps; the existing callers do not pass it): the e-greedy draw of agent.py:58-59 for row
// `rng_row` happens here, in the thread that stores the action — rb_eps_draw below; q stays the GREEDY action's value.
struct rb_eps_choice {
  int explore;      // u < epsilon
  int action;       // x1 % A (meaningful when explore)
};
// (x0, x1, ., .) = Philox4x32-10(key = seed, counter = (lo = round, hi = row)); u = (x0 >> 8) * 2^-24 in [0, 1); counter-based,
// nothing is stored: the same (seed, round, row) always gives the same draw
__device__ __forceinline__ rb_eps_choice rb_eps_draw(uint64_t seed, uint64_t round, int row, float epsilon, int A) {
  const rb_philox_out r = rb_philox(seed, (uint64_t)row, round);
  const float u = (float)(r.v[0] >> 8) * 0x1p-24f;
  rb_eps_choice c;
  c.explore = u < epsilon ? 1 : 0;
  c.action = (int)(r.v[1] % (uint32_t)A);
  return c;
}
__device__ __forceinline__ void rb_head_act_body(int Z, int A, const float* lg, const float* support, float* s_mean, float* s_ev,
                                                 int32_t* action_out, float* q_out, const unsigned* err, unsigned err_epoch = 0u,
                                                 float epsilon = -1.0f, uint64_t rng_seed = 0, uint64_t rng_round = 0, int rng_row = 0,
                                                 uint8_t* explored_out = nullptr) {
  const int t = (int)threadIdx.x;
  const int lane = rb_lane(), wave = rb_wave(), nw = (int)(blockDim.x >> 6);
  for (int z = t; z < Z; z += (int)blockDim.x) {
    float acc = 0.0f;
    for (int a = 0; a < A; ++a) acc += lg[Z + a * Z + z];
    s_mean[z] = acc / (float)A;
  }
  __syncthreads();
  for (int a = wave; a < A; a += nw) {
    float mx = -INFINITY;
    for (int z = lane; z < Z; z += 64) mx = fmaxf(mx, rb_dueling_q(lg, s_mean, Z, a, z));
    mx = rb_wave_max(mx);
    float se = 0.0f, sv = 0.0f;
    for (int z = lane; z < Z; z += 64) {
      const float e = expf(rb_dueling_q(lg, s_mean, Z, a, z) - mx);
      se += e;
      sv += support[z] * e;
    }
    se = rb_wave_sum(se);
    sv = rb_wave_sum(sv);
    if (lane == 0) s_ev[a] = sv / se;
  }
  __syncthreads();
  if (t == 0) {
    int best = 0;
    float bv = s_ev[0];
    for (int a = 1; a < A; ++a)
      if (s_ev[a] > bv) { bv = s_ev[a]; best = a; }
#if defined(RB_HOST_INTERP)
    if (err && err_epoch != 0u && *err == err_epoch) best = -1;
#else
    if (err && err_epoch != 0u && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == err_epoch) best = -1;   // a bounded in-launch wait of THIS launch expired: no action
#endif
    if (epsilon >= 0.0f) {
      const rb_eps_choice c = rb_eps_draw(rng_seed, rng_round, rng_row, epsilon, A);
      if (c.explore && best >= 0) best = c.action;
      if (explored_out) *explored_out = (uint8_t)c.explore;
    }
#if !defined(RB_HOST_INTERP)
    // (action, q) as ONE aligned 8-byte word where the caller laid them out that way (rainbow_amd/agent.py _forward_single: a pinned
    // pair): a single system-scope store — both are there when the host sees the action change, and the launch ends one host-memory
    // round trip earlier than with q, a system-scope fence, then the action (round 6: ~1 us of act()'s 39)
    if (action_out && q_out && reinterpret_cast<const void*>(q_out) == reinterpret_cast<const void*>(action_out + 1) &&
        (reinterpret_cast<uintptr_t>(action_out) & 7u) == 0) {
      const unsigned long long pack = (unsigned long long)(unsigned)best | ((unsigned long long)__builtin_bit_cast(unsigned, bv) << 32);
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(action_out), pack, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
#endif
    // q BEFORE the action, a system-scope fence in between: a host that polls the (pinned) action word for the value it
    // preset to change may read q right after
    if (q_out) *q_out = bv;
#if !defined(RB_HOST_INTERP)
    __threadfence_system();
#endif
    if (action_out) *action_out = best;
  }
}
