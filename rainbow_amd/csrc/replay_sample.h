// replay_sample.h — ReplayMemory.sample and update_priorities on the device: the window of one sample, the sampler proper
// (rb_sample_main), k_sample with its co-tenant workgroups, the frame-stack gather, k_update and the single-launch
// k_update_sample.  Included by replay.hip only, after noise_body.h and adam_body.h (the co-tenants' bodies).
#pragma once
#include "replay_search.h"
#include "replay_spec.h"

// Window, scalars and importance weight of ONE sample (memory.py:111-121,140-145,151-153) with every load of the window
// requested in a single batch: NCH chunks of 8 timesteps and 8 rewards (NCH = ceil((h + n) / 8): 1 for n = 3, 3 for the
// data-efficient n = 20 — whose second and third chunk used to be two more dependent round trips each).  n is the EFFECTIVE horizon
// v.n: the return, the nonterminal slot, the next-state slots and the blanking are those of a replay built with multi_step = n; the
// row of the window table keeps the stride history + n_max — word RB_STRIDE_SLOT of `scaling`, a load in the window's own batch —
// and its slots from h + n on are -1, never a ring index.
template <int NCH>
__device__ __forceinline__ float rb_sample_window(const ReplayView& v, int64_t idx, float prob, float p_total, int32_t full,
                                                  int64_t w_index, float neg_beta_f32, const float* scaling, int32_t* win,
                                                  int64_t* action_out, float* return_out, float* nonterminal_out) {
  // ring slots as 32-bit, wrapped with two selects (capacity > window, checked by the host; |offset| < capacity): the
  // 64-bit while-loop form put control flow between the loads, and every load became its own ~0.35 us round trip
  // (5.8 us for the 16 loads of n = 3, 16.8 us for the 48 loads of n = 20 — measured with in-kernel timestamps)
  // S interleaved streams (rb_replay_create_streams): window slot k of the sample is ring slot idx + k S — the same stream, k
  // transitions later.  The create-time check (h + n) S < C keeps every offset below C in magnitude, so the two selects still wrap.
  const int32_t C = (int32_t)v.capacity;
  const int32_t S = v.streams;
  const int32_t id = (int32_t)idx;
  const int h = v.history, n = v.n;
  const int win_len = h + n;
  int32_t win_stride = reinterpret_cast<const int32_t*>(scaling)[RB_STRIDE_SLOT];
  auto wrap = [C](int32_t x) { x += x < 0 ? C : 0; x -= x >= C ? C : 0; return x; };
  const int32_t first = id - (h - 1) * S;                             // window slot 0 (unwrapped)
  constexpr int NT = 8 * NCH;
  int ts[NT];
  float rw[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tc = t < win_len ? t : win_len - 1;
    ts[t] = v.timestep[wrap(first + tc * S)];
    const int kc = t < n ? t : n - 1;
    rw[t] = v.reward[wrap(id + kc * S)];
  }
  const int act_now = v.action[id];                                   // slot h-1 is never blanked
  const uint8_t nt_last = v.nonterminal[wrap(id + n * S)];
  // IS weight while those loads are in flight: probs / p_total ; capacity * probs ; ** -beta (memory.py:151-153).  The
  // reference evaluates the power in float32 (numpy: ~1 ulp, machine dependent); here exp(-beta * log(x)) in float64
  // (relative error ~1e-15, then ONE rounding to float32 — correctly rounded except on near-ties) — a third of the
  // instructions of the general double pow(), which was the longest ALU chain of the kernel.
  float w;
  {
    const float pn = __fdiv_rn(prob, p_total);
    const float cap = (float)(full ? C : w_index);
    const float base = __fmul_rn(cap, pn);
    w = base > 0.0f ? (float)exp((double)neg_beta_f32 * log((double)base)) : (float)pow((double)base, (double)neg_beta_f32);
  }
  unsigned long long first_bits = 0ull;  // h+n <= 64
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t < win_len && ts[t] == 0) first_bits |= 1ull << t;
  unsigned long long blank = 0ull;
  for (int t = h - 2; t >= 0; --t) {  // memory.py:116-117
    const bool b = ((blank >> (t + 1)) & 1ull) || ((first_bits >> (t + 1)) & 1ull);
    if (b) blank |= 1ull << t;
  }
  for (int t = h; t < win_len; ++t) {  // memory.py:118-119
    const bool b = ((blank >> (t - 1)) & 1ull) || ((first_bits >> t) & 1ull);
    if (b) blank |= 1ull << t;
  }
  // (the stride was requested in front of the window's loads and is first USED here, next to the stores that need it: the
  // empty statement keeps the row address from being formed, and the load from being waited for, in the middle of the batch)
#if !defined(RB_HOST_INTERP)
  asm volatile("" : "+v"(win_stride));
#endif
  int32_t* my_win = win + (int64_t)threadIdx.x * win_stride;            // thread i = sample i
  for (int t = 0; t < win_len; ++t) my_win[t] = ((blank >> t) & 1ull) ? -1 : wrap(first + t * S);
  for (int t = win_len; t < win_stride; ++t) my_win[t] = -1;          // the row's tail: -1 like a blanked slot, never a ring index
  *action_out = (int64_t)act_now;                                     // memory.py:140
  float R = 0.0f;                                                     // memory.py:142-143, k ascending
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    if (k < n) {
      const float rew = ((blank >> (h - 1 + k)) & 1ull) ? 0.0f : rw[k];
      R = __fadd_rn(R, __fmul_rn(rew, scaling[k]));
    }
  }
  *return_out = R;
  const int t_last = h + n - 1;                                       // memory.py:145
  *nonterminal_out = ((blank >> t_last) & 1ull) ? 0.0f : (nt_last ? 1.0f : 0.0f);
  return w;
}

// ReplayMemory.sample on device (memory.py:124-155).  ONE workgroup, thread i = sample i
// (batch <= 1024).  The rejection loop (memory.py:128-132) runs inside the kernel so the
// steady-state learn step has no host round trip.
#if defined(RB_STAMP)
__device__ long long g_stamp[32];
#define RB_STAMP_AT(i) do { if (threadIdx.x == 0 && blockIdx.x == 0) g_stamp[i] = wall_clock64(); } while (0)
#else
#define RB_STAMP_AT(i) ((void)0)
#endif
// MAXT = 256 for batches up to 256 (the learn step's shapes): the register budget of a 4-wave workgroup lets a thread hold
// a six-level subtree; MAXT = 1024 (batches up to 1024) keeps to four levels per trip and 128 registers.  NO variant may
// spill: a kernel with a scratch segment slowed every kernel of the step on MI355X (214 -> 283 us per step, measured).
// AU = float4 quadruples per thread of the hosted optimiser workgroups (adam_body.h): they inherit this kernel's register
// allocation, i.e. 2 waves per SIMD under the 256-thread variant's 205 VGPRs (needs AU = 8 to keep enough bytes in flight:
// 42 us per hosted launch against 46 with AU = 4) and 4 under the 1024-thread variant's 127 (AU = 4)
#define RB_HOST_AU_WIDE 4      // quadruples per hosted thread under the 1024-thread variant (5 spills under its 128-register cap)
// (optimizer_host.h clip_adam_impl sizes the pending pass for 4 quadruples per plain thread and 2 (mu, sigma) pairs per pair thread — pair_blk0 and
// the pair grid in clip_adam_impl; the hosting launch rescales the block count by this constant: any other value would split
// plain and pair workgroups differently from what the pass expects)

// The sampler proper (one workgroup, thread i = sample i): shared by k_sample (block 0) and k_update_sample.  top_staged: the
// caller has already copied the tree top into s_top (and kept it current).
template <int MAXT>
__device__ __forceinline__ void rb_sample_main(const ReplayView& v, int32_t batch, float neg_beta_arg, const float* neg_beta_ptr,
                                               const double* unit_uniforms, int32_t max_attempts, uint64_t seed, const float* scaling,
                                               int64_t* tree_idx_out, int32_t* win, int64_t* actions_out, float* returns_out,
                                               float* nonterminals_out, float* weights_out, int32_t* fail_count, int32_t lds_top,
                                               int* s_flag, float* s_red, float* s_top, bool top_staged, SpecResult* spec,
                                               unsigned spec_epoch) {
  RB_STAMP_AT(0);
  const int i = (int)threadIdx.x;
  const bool active = i < batch;
  const int64_t C = v.capacity;
  const int h = v.history, n = v.n;
  const float neg_beta_f32 = neg_beta_ptr ? *neg_beta_ptr : neg_beta_arg;

  const int n_cached = (int)(v.tree_len < RB_TOP_NODES ? v.tree_len : RB_TOP_NODES);
  if (lds_top && !top_staged) rb_stage_top(s_top, v.tree, n_cached);
  const int64_t w_index = v.hdr->index;
  const int32_t full = v.hdr->full;
  const uint64_t rng_base = v.hdr->rng_counter;
  const float p_total_g = v.tree[0];
  // Validity of slot idx (memory.py:131) per stream, without a division: with S streams the write head is J S and idx = j S + s,
  // and the rule is (J - j) mod Cs > n and (j - J) mod Cs >= h (Cs = C / S).  With d = (index - idx) mod C and e = (idx - index)
  // mod C that is exactly  n S < d <= C - S  and  e >= h S  (d = m S - s for m = (J - j) mod Cs >= 1; m = 0 puts d in
  // (C - S, C); e = ((j - J) mod Cs) S + s).  S = 1 gives the reference's two tests unchanged.
  const int64_t v_near = (int64_t)n * v.streams, v_far = C - v.streams, v_hist = (int64_t)h * v.streams;
  if (lds_top) __syncthreads();
  RB_STAMP_AT(1);
  const float p_top0 = s_top[0];                                // (an unconditional LDS read: as an operand of the select below the
                                                                //  compiler formed a generic pointer and the kernel's only flat load)
  const float p_total = lds_top ? p_top0 : p_total_g;           // memory.py:149
  // segment_length = p_total / batch_size: float32 / python int -> float32 (NEP 50)
  const float seg_f = __fdiv_rn(p_total, (float)batch);         // memory.py:125
  const double seg = (double)seg_f;
  const double start = __dmul_rn((double)i, seg);               // memory.py:126 (int64 * f32 -> f64)

  int64_t leaf = v.tree_start;
  float prob = 0.0f;
  int attempt = 0;
  int ok = 0;
  for (; attempt < max_attempts; ++attempt) {
    double u;
    if (unit_uniforms) {
      u = active ? unit_uniforms[(int64_t)attempt * batch + i] : 0.0;
    } else {
      const rb_philox_out r = rb_philox(seed, rng_base + (uint64_t)attempt, (uint64_t)i);
      u = rb_u53(r.v[0], r.v[1]);
    }
    // np.random.uniform(0.0, seg, B) = 0.0 + seg*u ; + segment_starts   (memory.py:129)
    const double sample = __dadd_rn(__dadd_rn(0.0, __dmul_rn(seg, u)), start);
    int valid = 1;
    if (active) {
      leaf = lds_top ? rb_tree_descend_fast(v.tree, s_top, n_cached, v.levels, v.tree_len, sample, &prob)
                     : rb_tree_descend_global<(MAXT <= 256 ? 6 : 4)>(v.tree, v.levels, v.tree_len, sample, &prob);   // memory.py:130
      const int64_t idx = leaf - v.tree_start;
      // memory.py:131, per stream (see v_far above): with S = 1 the second bound is d <= C - 1, always true
      const int64_t d = rb_wrap(w_index, -idx, C);
      valid = (d > v_near) && (d <= v_far) && (rb_wrap(idx, -w_index, C) >= v_hist) && (prob != 0.0f);
    }
    RB_STAMP_AT(2);
    ok = rb_block_all(valid, s_flag);
    if (ok) break;
  }
  RB_STAMP_AT(3);
  const int attempts_used = ok ? attempt + 1 : max_attempts;

  // ---- window (memory.py:111-121), scalars (memory.py:140-145), IS weights (151-154)
  float w = 0.0f;
  if (active) {
    const int64_t idx = leaf - v.tree_start;
    const int win_len = h + n;
    float nt_f;
    const int nch = (win_len + 7) >> 3;                                 // block-uniform (of the effective window, not the stride)
#define RB_WIN(N) w = rb_sample_window<N>(v, idx, prob, p_total, full, w_index, neg_beta_f32, scaling, win, &actions_out[i], &returns_out[i], &nt_f)
    if (nch <= 1) RB_WIN(1);
    else if (nch <= 3 || MAXT > 256) RB_WIN(3);      // (the 1024-thread variant has no registers for longer windows in one batch ...
    else RB_WIN(8);                                  //  ... rb_replay_sample refuses batch > 256 with history + multi_step > 24)
#undef RB_WIN
    nonterminals_out[i] = nt_f;
    // a draw that gave up marks its own index buffer: the write-back of THIS buffer's batch is dropped (rb_update_body), no other
    tree_idx_out[i] = ok ? leaf : (int64_t)-1;
  }
  RB_STAMP_AT(4);
  const float w_max = rb_block_max(active ? w : -INFINITY, s_red);
  // The reference retries until a batch is valid (memory.py:128-132); this loop is bounded.  If the bound is hit (a
  // buffer too small for the batch: some stratum lies inside the write head's exclusion zone) the last draw is NOT a
  // legal batch — windows may straddle the write head and a zero-priority leaf would give w = inf.  Make it harmless:
  // every importance weight is 0, so the step's gradient is exactly zero, and the failure is counted in host-visible
  // memory (rb_replay_failed_samples) so the caller can raise without a device synchronisation.
  if (active) weights_out[i] = ok ? __fdiv_rn(w, w_max) : 0.0f;         // memory.py:154
  if (spec) {
    // a TENTATIVE draw (rb_replay_spec_launch): the header is not touched — what the draw would have done to it goes to the side
    // record, committed by the draw that accepts it (k_sample, spec_mode 2), and published last (rb_spec_publish).
    if (threadIdx.x == 0) {
      spec->attempts = attempts_used;
      spec->status = ok ? 0 : 1;
      spec->rng_next = rng_base + (uint64_t)attempts_used;
    }
#if !defined(RB_HOST_INTERP)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    __syncthreads();
    if (threadIdx.x == 0) rb_spec_publish(spec, spec_epoch);
    return;
  }
  if (threadIdx.x == 0) {
    v.hdr->last_attempts = attempts_used;
    v.hdr->last_status = ok ? 0 : 1;
    if (!unit_uniforms) v.hdr->rng_counter = rng_base + (uint64_t)attempts_used;
    // (a system-scope atomic on the kernel-argument pointer: a global instruction; the former volatile read-modify-write was
    // compiled to flat loads/stores)
    if (!ok && fail_count) rb_atomic_inc_system(fail_count);
  }
  RB_STAMP_AT(5);
}

// EMA: the hosted pass also moves the target network (adam_body.h; arguments with a target pointer).  An instantiation of its
// own, chosen by sample_impl from the job: the plain one stays the kernel it was, register for register.
template <int MAXT, int AU, bool EMA = false>
__global__ __launch_bounds__(MAXT) void k_sample(ReplayView v, int32_t batch, float neg_beta_arg,
                                                  const float* neg_beta_ptr, const double* unit_uniforms, int32_t max_attempts, uint64_t seed,
                                                  const float* scaling, int64_t* tree_idx_out, int32_t* win,
                                                  int64_t* actions_out, float* returns_out, float* nonterminals_out,
                                                  float* weights_out, const NoiseJob* job_dev, float* job_noise, float* job_noise2,
                                                  unsigned long long* job_ctr, int32_t* fail_count, int32_t lds_top,
                                                  int32_t noise_blocks, const ClipAdamArgs* adam_dev, SpecResult* spec,
                                                  unsigned spec_epoch, int32_t spec_mode) {
  if ((int)blockIdx.x > noise_blocks) {
    // co-tenant workgroups behind the noise ones: the previous learn call's optimiser pass (adam_body.h) — independent of
    // this batch's sampling, and 30 us of pure streaming that now runs beside the sampler's serial chain, not before it
    __shared__ float s_adam[18];
#if defined(RB_STAMP)       // slots 6 / 7: start of the first / last hosted workgroup, slot 8: the latest end of any of them
    if (threadIdx.x == 0 && (int)blockIdx.x == noise_blocks + 1) g_stamp[6] = wall_clock64();
    if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1) g_stamp[7] = wall_clock64();
#endif
    rb_adam_hosted_block<AU, EMA>(adam_dev, (int)blockIdx.x - 1 - noise_blocks, (int)gridDim.x - 1 - noise_blocks, s_adam);
#if defined(RB_STAMP)
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned long long*>(&g_stamp[8]), (unsigned long long)wall_clock64());
#endif
    return;
  }
  if (blockIdx.x > 0) {   // co-tenant workgroups: the learner's noise resample (no dependency on the sampler)
    // the job's SCALARS are read here, from device memory: as a by-value kernel argument its 30 SGPRs were live across the
    // sampler path as well, 17 SGPRs spilled and the kernel carried a private segment (no kernel of the step may: DESIGN.md
    // §6).  Its three POINTERS stay kernel arguments: a pointer loaded from memory is a generic pointer and every access
    // through it a FLAT instruction — this was the only kernel of the library with flat instructions.
    // (field by field, the map by reference: a local copy of the struct would be a dynamically indexed stack object)
    const int nb = (int)blockIdx.x - 1, nblk = job_dev->nblk;
    rb_noise_body(job_noise, job_noise2, nullptr, job_dev->map, job_dev->seed, job_ctr, nb % nblk, nblk, nb / nblk, job_dev->nets);
    return;
  }
  __shared__ int s_flag[16];
  __shared__ float s_red[16];
  __shared__ __attribute__((aligned(16))) float s_top[RB_TOP_NODES + 1];
  if (spec_mode >= 2) {               // an early draw is in flight: accept it (2) or wait and draw (3) — replay_spec.h
    if (threadIdx.x == 0) {           // ONE lane waits, decides and commits (the decision goes to the others through LDS)
      int accept = rb_poll_epoch(&spec->done, spec_epoch, fail_count ? fail_count + 2 : nullptr);
      if (spec_mode != 2 || spec->status == RB_SPEC_ABORTED) accept = 0;
      if (accept) {
        const int32_t st = spec->status;
        v.hdr->last_attempts = spec->attempts;
        v.hdr->last_status = st;
        v.hdr->rng_counter = spec->rng_next;
        if (st != 0 && fail_count) rb_atomic_inc_system(fail_count);
      }
      s_flag[15] = accept;
    }
    __syncthreads();
    if (s_flag[15]) return;                               // block-uniform
    __syncthreads();                                      // (s_flag is reused by the sampler proper)
  }
  rb_sample_main<MAXT>(v, batch, neg_beta_arg, neg_beta_ptr, unit_uniforms, max_attempts, seed, scaling, tree_idx_out, win, actions_out,
                       returns_out, nonterminals_out, weights_out, fail_count, lds_top, s_flag, s_red, s_top, false,
                       spec_mode == 1 ? spec : nullptr, spec_epoch);
}

// Frame-stack gather (memory.py:136-138 minus the /255): block = (sample, stack slot),
// 441 sixteen-byte lanes per 7056-byte frame, zero fill for blanked slots.
// Stream-agnostic: the ring slot of every frame comes from the sampler's window table, which already holds the stream's
// stride (rb_sample_window); the learner's zero-copy conv path reads the ring through the same table.
__global__ __launch_bounds__(256) void k_gather_stacks(ReplayView v, int32_t batch, const int32_t* win, int32_t win_stride,
                                                        uint8_t* states, uint8_t* next_states) {
  constexpr int VEC = RB_FRAME_BYTES / 16;
  const int h = v.history, n = v.n;
  const int per_sample = 2 * h;
  for (int b = (int)blockIdx.x; b < batch * per_sample; b += (int)gridDim.x) {
    const int i = b / per_sample;
    const int s = b % per_sample;
    const bool is_next = s >= h;
    const int c = is_next ? s - h : s;
    const int slot = is_next ? n + c : c;
    const int32_t ring = win[(int64_t)i * win_stride + slot];
    uint4* d = (uint4*)((is_next ? next_states : states) + ((int64_t)i * h + c) * RB_FRAME_BYTES);
    if (ring < 0) {
      const uint4 z = make_uint4(0u, 0u, 0u, 0u);
      for (int t = (int)threadIdx.x; t < VEC; t += (int)blockDim.x) d[t] = z;
    } else {
      const uint4* src = (const uint4*)(v.frames + (int64_t)ring * RB_FRAME_BYTES);
      for (int t = (int)threadIdx.x; t < VEC; t += (int)blockDim.x) d[t] = src[t];
    }
  }
}

// ---------------------------------------------------------------------- update --
// (body: replay_update.h)
__global__ __launch_bounds__(1024) void k_update(ReplayView v, const int64_t* tree_idx, const float* values, int32_t n,
                                                  int32_t apply_pow, double omega) {
  __shared__ float lds[UpdateLds<2048, 1024>::WORDS];
  rb_update_auto<2048, 1024>(v, tree_idx, values, n, apply_pow, omega, lds);
}

// ------------------------------------------------------------ update + sample --
// update_priorities(idx_k, loss_k) followed by sample(k + 1) — the PER loop of memory.py:148-159 / agent.py:62,100 — as ONE
// launch of one workgroup: the two are a dependent pair of single-workgroup latency chains, and as two launches the second
// pays a launch boundary, re-reads the header and stages the 16 KB tree top that the first has just rewritten.  Here the top
// is staged while the update's operands are in flight, the sorted-batch update (rb_update_sorted_wave, one wave) patches that
// LDS copy as it writes the tree, and the search starts from it.  Unsorted or longer batches (<= 256) take the hashed body
// and the top is staged afterwards.  Same arithmetic, same order: tree, header and batch are bit-identical to the two calls.
__global__ __launch_bounds__(256) void k_update_sample(ReplayView v, const int64_t* upd_idx, const float* upd_val, int32_t upd_n,
                                                        int32_t apply_pow, double omega, int32_t batch, float neg_beta_arg,
                                                        const float* neg_beta_ptr, const double* unit_uniforms, int32_t max_attempts,
                                                        uint64_t seed, const float* scaling, int64_t* tree_idx_out, int32_t* win,
                                                        int64_t* actions_out, float* returns_out, float* nonterminals_out,
                                                        float* weights_out, int32_t* fail_count, SpecResult* spec, unsigned spec_epoch) {
  __shared__ int s_flag[16];
  __shared__ float s_red[16];
  __shared__ __attribute__((aligned(16))) float s_top[RB_TOP_NODES + 1];
  __shared__ float lds_upd[UpdateLds<512, 256>::WORDS];
  __shared__ int s_sorted;
  const int i = (int)threadIdx.x;
  if (spec) {
    // the early pair (rb_replay_spec_launch): the gate in front of this launch (same stream) waited for the head kernel of the learn
    // call whose losses are written back here.  If the gate EXPIRED the losses may not be final: give up — no write-back (counted as a
    // dropped one), no draw; the record says so and the accepting sampler launch draws itself (k_sample, spec_mode 2)
    if (i == 0) {
#if defined(RB_HOST_INTERP)
      s_flag[0] = spec->abort_epoch == spec_epoch ? 1 : 0;
#else
      s_flag[0] = __hip_atomic_load(&spec->abort_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == spec_epoch ? 1 : 0;
#endif
    }
    __syncthreads();
    const int aborted = s_flag[0];
    __syncthreads();
    if (aborted) {                                        // block-uniform
      if (i == 0) {
        spec->attempts = 0; spec->status = RB_SPEC_ABORTED;
        if (v.dropped) rb_atomic_inc_system(v.dropped);
        rb_spec_publish(spec, spec_epoch);
      }
      return;
    }
  }
  const int n_cached = (int)(v.tree_len < RB_TOP_NODES ? v.tree_len : RB_TOP_NODES);
  UpdateOperand op;
  op.node = -1; op.val = 0.0f; op.status = 0; op.sorted = 0;
  if (upd_n <= 64) {
    if (i < 64) op = rb_update_load(v, upd_idx, upd_val, upd_n);
    if (i == 0) s_sorted = op.sorted;
  } else if (i == 0) {
    s_sorted = 0;
  }
  rb_stage_top(s_top, v.tree, n_cached);
  __syncthreads();
  const bool sorted = s_sorted != 0;                                       // block-uniform
  if (sorted) {
    if (i < 64) rb_update_sorted_wave(v, op, upd_n, apply_pow, omega, s_top, n_cached);
  } else {
    rb_update_body<512, 256>(v, upd_idx, upd_val, upd_n, apply_pow, omega, lds_upd);
  }
  __threadfence_block();               // the tree this workgroup wrote, read back by the same workgroup (as in k_rebuild_top)
  __syncthreads();
  rb_sample_main<256>(v, batch, neg_beta_arg, neg_beta_ptr, unit_uniforms, max_attempts, seed, scaling, tree_idx_out, win, actions_out,
                      returns_out, nonterminals_out, weights_out, fail_count, 1, s_flag, s_red, s_top, sorted, spec, spec_epoch);
}
