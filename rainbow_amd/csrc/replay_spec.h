// replay_spec.h — the device side of the early draw (host side: replay.hip rb_replay_spec_launch / sample_impl; interface for
// the learner: replay_internal.h).  Included by replay.hip only.
//
// ReplayMemory.update_priorities of learn call k and ReplayMemory.sample of call k + 1 (agent.py:100 / :63, memory.py:124-159) depend
// on nothing of call k after its head kernel (the per-sample loss), while call k's backward is another ~90 us of launches that
// never touch the replay.  rb_replay_spec_launch issues that pair on a stream the replay owns, as soon as the head is done:
// the write-back is final (it IS call k's), the draw TENTATIVE — it writes the caller's sample buffers and the replay's OTHER
// window table, but its header effects (Philox counter, status, attempts, failure count) go to a side record.  The next draw on
// the handle with the same arguments ACCEPTS it (k_sample block 0 waits for the record's epoch, commits the header effects and
// returns); any other entry point that touches the replay waits for the stream and discards it; a draw with other arguments
// waits and draws again.  Results are those of the two calls made one after the other.
//
// k_sample's spec_mode: 1 = THIS is the tentative draw; 2 = an early draw is in flight on another stream and is accepted: wait for
// it, commit its header effects, done; 3 = in flight but not acceptable (other arguments, or a public entry point): wait, then draw
// as usual.  FAIL SAFE: when the wait expires, or the pair on the other stream reports that it gave up (SPEC_ABORTED: its gate
// expired), mode 2 draws here as well — the header was never touched by the tentative draw, so this is exactly the draw a launch
// without an early draw would have made.
#pragma once
#include "replay_internal.h"

#define RB_SPEC_ABORTED 2     // SpecResult.status: the pair gave up (its gate expired) — nothing was written back, nothing was drawn
struct SpecResult {
  unsigned long long rng_next;
  int32_t attempts, status;  // status: 0 = a legal batch, 1 = the draw hit its attempt bound, RB_SPEC_ABORTED
  unsigned done;             // epoch of the last tentative draw that completed (release-stored last)
  unsigned abort_epoch;      // epoch of the last pair whose gate (k_spec_gate) expired
};

// wait for *flag >= epoch (ONE lane polls, relaxed; then one agent-scope acquire; the caller broadcasts).  Returns 1 when the flag
// arrived, 0 when the bound (RB_WAIT_EPOCH_POLLS polls, ~2 ms) expired — counted in *err_host.  The producers are launches submitted
// EARLIER (a head kernel, an early draw), so an expiry means something serialises the two queues against each other (a profiler's
// counter pass does) or the device is wedged; every caller FAILS SAFE: it does the work in its own launch instead (k_sample) or
// drops it and says so (k_spec_gate -> k_update_sample), never proceeds on data that may not be final.
#define RB_WAIT_EPOCH_POLLS (1u << 13)
// (the polling lane's part: returns 1 when the flag arrived; ends with the agent-scope acquire either way)
__device__ __forceinline__ int rb_poll_epoch(const unsigned* flag, unsigned epoch, int32_t* err_host) {
#if defined(RB_HOST_INTERP)
  const int ok = (int)(*flag - epoch) >= 0;             // launches run in submission order there
  if (!ok && err_host) *err_host = *err_host + 1;
  return ok;
#else
  unsigned spins = 0;
  int ok = 1;
  while ((int)(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - epoch) < 0) {
    __builtin_amdgcn_s_sleep(8);
    if (++spins > RB_WAIT_EPOCH_POLLS) { ok = 0; if (err_host) rb_atomic_inc_system(err_host); break; }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return ok;
#endif
}

// The record's epoch, stored LAST behind an agent-scope release of everything the calling workgroup wrote (ONE lane calls): the
// accepting workgroup polls it from another stream (rb_poll_epoch).
__device__ __forceinline__ void rb_spec_publish(SpecResult* spec, unsigned epoch) {
#if defined(RB_HOST_INTERP)
  spec->done = epoch;
#else
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(&spec->done, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// One wave, no LDS, a handful of registers: holds the replay's stream back until *flag >= epoch.  The early pair itself must not
// do the waiting: submitted a whole step ahead of the device, a 256-thread / 50 KB workgroup polling on a CU takes that CU away
// from every launch of the step that needs all 256 (the batch-256 conv kernels are one LDS-filling workgroup per CU: each of them
// ran a second round for ONE workgroup — 498 -> 650 us per step, measured); a lone wave fits beside anything.
__global__ __launch_bounds__(64) void k_spec_gate(const unsigned* flag, unsigned epoch, int32_t* err_host, SpecResult* spec, unsigned spec_epoch) {
  // (ONE wave, no LDS, no barrier: with a shared word the gate stopped fitting beside the LDS-filling conv workgroups of batch 256 —
  // every conv launch ran a second round for the one workgroup of the gate's CU: 498 -> 537 us per step, round6_second_trace_b256_spec)
  if (threadIdx.x != 0) return;
  if (!rb_poll_epoch(flag, epoch, err_host)) {
    // the head kernel's launch was not seen to complete within the bound: the pair behind this gate must NOT read its losses.  It is
    // told to give up (k_update_sample: no write-back — counted as dropped — and no draw; the accepting launch draws itself)
#if defined(RB_HOST_INTERP)
    spec->abort_epoch = spec_epoch;
#else
    __hip_atomic_store(&spec->abort_epoch, spec_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
  }
}
