// stats_common.h — what the two read-out kernels (learn_stats.h k_step_stats, replay_stats.h k_priority_stats) share: values
// that one workgroup hands to the LAST workgroup of the same launch, and the ticket that tells a workgroup it is that one.
//
// Both kernels spread their rows / leaves over workgroups, each of which leaves a few per-workgroup values in a scratch the
// handle owns; the last workgroup to take a ticket folds them in a fixed order, so the result does not depend on which
// workgroup that is.  The ticket is noise_body.h's (fence, add, the last arrival puts the counter back to zero: no memset
// between launches, the scratch is zeroed once when it is allocated), with the payload on the agent-coherent path on both sides:
// the 8 XCDs have private L2s, so a plain store may still sit dirty in the writer's L2 — or a stale line in the reader's —
// when the ticket says "everybody has arrived".  Plain C++ throughout: relaxed agent-scope atomic stores / loads are
// write-through stores / coherent loads on gfx950, and __threadfence() is the agent-scope fence.
#pragma once
#include "rb_common.h"

__device__ __forceinline__ void rb_pub_f64(double* p, double v) {
#if defined(RB_HOST_INTERP)
  *p = v;
#else
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
__device__ __forceinline__ double rb_sub_f64(const double* p) {
#if defined(RB_HOST_INTERP)
  return *p;
#else
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
__device__ __forceinline__ void rb_pub_f32(float* p, float v) {
#if defined(RB_HOST_INTERP)
  *p = v;
#else
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
__device__ __forceinline__ float rb_sub_f32(const float* p) {
#if defined(RB_HOST_INTERP)
  return *p;
#else
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// All threads of the workgroup call, after their rb_pub_* stores and global atomics.  Returns true, block-uniform, in the last of
// the `expected` workgroups of the launch to arrive: everything the others published is then visible to rb_sub_* loads and
// to global atomics.  Every thread fences for its own stores (a fence waits for the stores of its own wave only).
__device__ __forceinline__ bool rb_last_arrival(unsigned* counter, unsigned expected, int* s_flag) {
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    const unsigned old = atomicAdd(counter, 1u);
    const int last = old + 1u == expected ? 1 : 0;
    if (last) atomicExch(counter, 0u);
    *s_flag = last;
  }
  __syncthreads();
  const bool last = *s_flag != 0;
  if (last) __threadfence();
  return last;
}
