// head.h — the C51 head of the learn step (k_head) and of Agent.act (k_head_act).  Included by learner.hip only.
#pragma once
#include "learner_internal.h"
#include "act_head.h"
#include "kernel_stamp.h"

// ------------------------------------------------------------------------- head --
// One workgroup per sample b.  Dueling combine (model.py:74-75), log-softmax of
// the taken action (agent.py:66-67), double-Q argmax on the online net (agent.py:71-73), target
// probabilities of that action (agent.py:75-76), C51 projection with the atom bins staged in LDS
// and accumulated in the reference's order (agent.py:79-92), cross-entropy (agent.py:94) and
// d loss / d logits for mean(w * loss) (agent.py:96).
#define RB_MAX_ATOMS 256
#define RB_MAX_ACTIONS 64


// One workgroup per sample.  The three logit rows (3*(Z + A*Z) floats) are pulled into LDS with one coalesced sweep; after
// that the kernel touches global memory only for its outputs.  ALL softmaxes of the sample are independent tasks spread over
// the waves in ONE phase: the A double-Q softmaxes of online(next_states) (agent.py:71-73), the A candidate softmaxes of
// target(next_states) — computed for every action while a* is still unknown instead of for a* alone afterwards (round 3's
// per-workgroup timeline: 1.4 us double-Q, then 2.0 us for the two remaining softmaxes on two of eight waves) — and the
// log-softmax of online(states)[action].  Every reduction over atoms is a wave64 DPP reduction (each lane owns atoms
// z = lane, lane + 64, ...; ZI = ceil(Z / 64) is a template parameter: 51 atoms are ONE slot per lane, the former fixed four
// slots quadrupled the instruction count of a phase that runs at one lone wave's issue rate).
#define RB_MAX_NZ RB_HEAD_MAX_NZ

template <int ZI>
struct HeadWave {
  int lane;
  // dueling mean over actions for this lane's atoms: a.mean(1)            model.py:75
  __device__ void mean_of(const float* lg, int Z, int A, float* mean) const {
#pragma unroll
    for (int i = 0; i < ZI; ++i) {
      const int z = lane + 64 * i;
      float acc = 0.0f;
      if (z < Z)
        for (int a = 0; a < A; ++a) acc += lg[Z + a * Z + z];
      mean[i] = acc / (float)A;
    }
  }
  // e[i] = exp(q - max), qm[i] = q - max for this lane's atoms; returns the wave-wide sum of e
  __device__ float softmax_of(const float* lg, int Z, const float* mean, int a, float* e, float* qm) const {
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < ZI; ++i) {
      const int z = lane + 64 * i;
      qm[i] = z < Z ? (lg[z] + lg[Z + a * Z + z]) - mean[i] : -INFINITY;   // q = v + a - mean_a(a)
      mx = fmaxf(mx, qm[i]);
    }
    mx = rb_wave_max(mx);
    float se = 0.0f;
#pragma unroll
    for (int i = 0; i < ZI; ++i) {
      const int z = lane + 64 * i;
      qm[i] = z < Z ? qm[i] - mx : 0.0f;
      e[i] = z < Z ? expf(qm[i]) : 0.0f;
      se += e[i];
    }
    return rb_wave_sum(se);
  }
};

struct HeadTenants {
  ConvWtJob job[2];
  int per_job;           // workgroups per job (0: no tenants)
};
#define RB_HEAD_THREADS 1024      // launch bound; the launch uses 64 x min(16, max(8, 2A + 1)) threads
template <int ZI>
__global__ __launch_bounds__(RB_HEAD_THREADS) void k_head(int B, int Z, int A, const float* logits, const int64_t* actions,
                                               const float* returns, const float* nonterminals, const float* weights,
                                               const float* support, float v_min, float v_max, float gamma_n,
                                               float delta_z, float* log_ps_a_out, float* pns_a_out, float* m_out,
                                               int32_t* a_star_out, float* loss_out, float* dlogits, long long* step_ctr,
                                               const int32_t* batch_status, int32_t* status_copy, float* dlogitsT, HeadTenants tn) {
  // tenant workgroups behind the B samples: the conv input-gradient kernels' weight operand of THIS step (conv_dx.h
  // rb_conv_wt_block) — independent of the head, on CUs this launch leaves idle (32 of 256 busy), two launches ahead of its
  // first reader
  if ((int)blockIdx.x >= B) {
    const int tb = (int)blockIdx.x - B;
    if (tb < tn.per_job) rb_conv_wt_block(tn.job[0], tb, tn.per_job);
    else rb_conv_wt_block(tn.job[1], tb - tn.per_job, tn.per_job);
    return;
  }
  __shared__ float s_lg[3][RB_MAX_NZ];               // rows: online(states), online(next), target(next)
  __shared__ float s_pt[RB_MAX_NZ];                  // target(next) probabilities of EVERY action: [a][z] at a * Z + z
  __shared__ float s_lo[RB_MAX_ATOMS], s_hi[RB_MAX_ATOMS], s_m[RB_MAX_ATOMS], s_logp[RB_MAX_ATOMS], s_sup[RB_MAX_ATOMS];
  __shared__ int s_l[RB_MAX_ATOMS], s_u[RB_MAX_ATOMS];
  __shared__ float s_ev[RB_MAX_ACTIONS];
  __shared__ float s_scal[2];                        // sum(m), -loss
  const int t = (int)threadIdx.x, T = (int)blockDim.x, lane = rb_lane(), wave = rb_wave(), nw = T >> 6;
  const int b = (int)blockIdx.x;
  const int NZ = Z + A * Z;
  RB_WGT(7, b, 0);
  RB_WGT_HW(7, b);
  for (int i = t; i < NZ; i += T) {
    s_lg[0][i] = logits[(int64_t)b * NZ + i];
    s_lg[1][i] = logits[(int64_t)(B + b) * NZ + i];
    s_lg[2][i] = logits[(int64_t)(2 * B + b) * NZ + i];
  }
  for (int z = t; z < Z; z += T) s_sup[z] = support[z];  // requested with the logits: one memory round trip, not two
  const float R = returns[b], nt = nonterminals[b], wgt = weights[b];
  const int act = (int)actions[b];
  __syncthreads();
  RB_WGT(7, b, 1);
  HeadWave<ZI> hw;
  hw.lane = lane;
  float mean[ZI], e[ZI], qm[ZI];

  // ---------------- every softmax of the sample, one task per wave (round-robin when 2A + 1 exceeds the wave count)
  for (int task = wave; task < 2 * A + 1; task += nw) {                 // wave-uniform
    if (task < A) {
      // double-Q selection on online(next_states)   agent.py:71-73
      hw.mean_of(s_lg[1], Z, A, mean);
      const float se = hw.softmax_of(s_lg[1], Z, mean, task, e, qm);
      float sv = 0.0f;
#pragma unroll
      for (int i = 0; i < ZI; ++i) sv += (lane + 64 * i < Z ? s_sup[lane + 64 * i] : 0.0f) * e[i];
      sv = rb_wave_sum(sv);
      if (lane == 0) s_ev[task] = sv / se;                            // sum_z z * p(z)
    } else if (task < 2 * A) {
      // target(next_states)[a] probabilities for candidate a   agent.py:75-76
      const int a = task - A;
      hw.mean_of(s_lg[2], Z, A, mean);
      const float se = hw.softmax_of(s_lg[2], Z, mean, a, e, qm);
#pragma unroll
      for (int i = 0; i < ZI; ++i) {
        const int z = lane + 64 * i;
        if (z < Z) s_pt[a * Z + z] = e[i] / se;
      }
    } else {
      // online(states): log p(s_t, a_t)            agent.py:66-67
      hw.mean_of(s_lg[0], Z, A, mean);
      const float se = hw.softmax_of(s_lg[0], Z, mean, act, e, qm);
      const float lse = logf(se);
#pragma unroll
      for (int i = 0; i < ZI; ++i) {
        const int z = lane + 64 * i;
        if (z < Z) {
          const float lp = qm[i] - lse;                             // log_softmax = (q - max) - log(sum exp(q - max))
          s_logp[z] = lp;
          log_ps_a_out[(int64_t)b * Z + z] = lp;
        }
      }
    }
  }
  __syncthreads();
  RB_WGT(7, b, 2);
  int a_star = 0;
  {
    float best = s_ev[0];
    for (int a = 1; a < A; ++a)
      if (s_ev[a] > best) { best = s_ev[a]; a_star = a; }         // argmax, first maximum
  }
  if (t == 0) a_star_out[b] = a_star;
  // this learn call's optimiser step number (1-based); a batch the sampler gave up on does not count (no update follows)
  if (b == 0 && t == 0) {
    const int32_t st = batch_status ? *batch_status : 0;
    if (status_copy) *status_copy = st;
    if (step_ctr && st == 0) *step_ctr = *step_ctr + 1;
  }
  // ---------------- projection inputs from the selected action's probabilities      agent.py:79-86
  for (int z = t; z < Z; z += T) {
    const float p = s_pt[a_star * Z + z];
    pns_a_out[(int64_t)b * Z + z] = p;
    float Tz = R + (nt * gamma_n) * s_sup[z];                 // agent.py:79
    Tz = fminf(fmaxf(Tz, v_min), v_max);                      // agent.py:80
    const float bq = (Tz - v_min) / delta_z;                  // agent.py:82
    int l = (int)floorf(bq), u = (int)ceilf(bq);              // agent.py:83
    if (u > 0 && l == u) l -= 1;                              // agent.py:85
    if (l < Z - 1 && l == u) u += 1;                          // agent.py:86
    s_l[z] = l; s_u[z] = u;
    s_lo[z] = p * ((float)u - bq);                            // agent.py:91
    s_hi[z] = p * (bq - (float)l);                            // agent.py:92
    s_m[z] = 0.0f;
  }
  __syncthreads();
  RB_WGT(7, b, 3);
  // ---------------- scatter into atom bins in the reference's accumulation order   agent.py:89-92
  // b is monotone in the atom index (support increasing, nt*gamma^n >= 0), so equal l (and equal u) form
  // contiguous runs: the first atom of a run owns its bin and adds the run left to right — exactly the order of
  // the reference's first index_add_ (all l bins, j ascending) followed by the second (u bins) on the same m.
  // The run's adds are inherently serial (float adds in the reference's order), but their OPERANDS need not be: walking the run with
  // `jj < Z && s_l[jj] == key` made every atom two dependent LDS round trips (~130 cycles), fine for the usual one to three atoms per
  // bin, 2 x 51 steps = 7 us for a TERMINAL transition, whose atoms all land in one bin — and with 256 samples per batch there is
  // almost always one: the launch was 12 us for 5.4 us workgroups (profiles/round6_wg_timeline_b256.txt).  For Z <= 64 the run lengths
  // come from one ballot of the run starts, and an owner fetches its run eight atoms per round trip, then adds them in order.
  const bool by_ballot = Z <= 64;
  auto scatter_runs = [&](const int* s_key, const float* s_x, bool second) {      // wave 0, lane = atom
    const bool valid = lane < Z;
    const int key = s_key[valid ? lane : Z - 1];
    const int prev = __shfl_up(key, 1);
    const bool start = valid && (lane == 0 || prev != key);
    const unsigned long long starts = __ballot(start ? 1 : 0);
    const unsigned long long rest = lane < 63 ? starts >> (lane + 1) : 0ull;       // run starts behind this atom
    const int len = rest ? __builtin_ctzll(rest) + 1 : Z - lane;                   // atoms of the run that starts here
    if (start) {
      float acc = second ? s_m[key] : 0.0f;
      for (int i0 = 0; i0 < len; i0 += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int jj = lane + i0 + u; v[u] = s_x[jj < Z ? jj : Z - 1]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = i0 + u < len ? acc + v[u] : acc;
      }
      s_m[key] = acc;
    }
  };
  {
    if (by_ballot) {
      if (wave == 0) scatter_runs(s_l, s_lo, false);
    } else {
      for (int j = t; j < Z; j += T) {
        const int key = s_l[j];
        if (j == 0 || s_l[j - 1] != key) {
          float acc = 0.0f;
          for (int jj = j; jj < Z && s_l[jj] == key; ++jj) acc += s_lo[jj];
          s_m[key] = acc;
        }
      }
    }
    __syncthreads();
    if (by_ballot) {
      if (wave == 0) scatter_runs(s_u, s_hi, true);
    } else {
      for (int j = t; j < Z; j += T) {
        const int key = s_u[j];
        if (j == 0 || s_u[j - 1] != key) {
          float acc = s_m[key];
          for (int jj = j; jj < Z && s_u[jj] == key; ++jj) acc += s_hi[jj];
          s_m[key] = acc;
        }
      }
    }
  }
  __syncthreads();
  RB_WGT(7, b, 4);
  for (int k = t; k < Z; k += T) m_out[(int64_t)b * Z + k] = s_m[k];
  if (wave == 0) {                                                // loss = -sum m * log p   agent.py:94
    float pl = 0.0f, pm = 0.0f;
    for (int z = lane; z < Z; z += 64) { pl += s_m[z] * s_logp[z]; pm += s_m[z]; }
    pl = rb_wave_sum(pl);
    pm = rb_wave_sum(pm);
    if (lane == 0) { s_scal[0] = pm; s_scal[1] = pl; loss_out[b] = -pl; }
  }
  __syncthreads();
  // ---------------- backward of mean(w * loss) to the logits     agent.py:96
  // d/dq[z] = (w/B) * (p[z] * sum(m) - m[z]) on the taken action; dueling adjoint:
  // dv[z] = g[z] ; da[a'][z] = (delta(a',act) - 1/A) * g[z]
  RB_WGT(7, b, 5);
  const float coef = wgt / (float)B;
  const float msum = s_scal[0];
  float* dl = dlogits + (int64_t)b * NZ;
  for (int i = t; i < NZ; i += T) {
    const int z = i < Z ? i : (i - Z) % Z;
    const float g = coef * (expf(s_logp[z]) * msum - s_m[z]);
    float o;
    if (i < Z) o = g;
    else o = ((i - Z) / Z == act ? g : 0.0f) - g / (float)A;
    dl[i] = o;
    if (dlogitsT) dlogitsT[(int64_t)i * B + b] = o;      // [NZ][B]: the output layer's input gradient reads 16 consecutive samples of a row
  }
  RB_WGT(7, b, 6);
}

// Agent.act / evaluate_q head (agent.py:53-55, 110-112) for ONE image at logits row `row` (act_head.h rb_head_act_body).
__global__ __launch_bounds__(256) void k_head_act(int Z, int A, const float* logits, int row, const float* support,
                                                   int32_t* action_out, float* q_out) {
  __shared__ float s_mean[RB_MAX_ATOMS];
  __shared__ float s_ev[RB_MAX_ACTIONS];
  row += (int)blockIdx.x;                       // batched acting: one workgroup per state, outputs indexed alike
  rb_head_act_body(Z, A, logits + (int64_t)row * (Z + A * Z), support, s_mean, s_ev, action_out ? action_out + blockIdx.x : nullptr,
                   q_out ? q_out + blockIdx.x : nullptr, nullptr);
}

// The same head with the e-greedy draw of agent.py:58-59 in it (rb_learner_act_batch_eps): workgroup i serves row0 + i of the
// caller's numbering, so a stream's draw does not depend on how the caller chunks its states.
__global__ __launch_bounds__(256) void k_head_act_eps(int Z, int A, const float* logits, const float* support, float epsilon,
                                                       uint64_t rng_seed, uint64_t rng_round, int row0, int32_t* action_out,
                                                       float* q_out, uint8_t* explored_out) {
  __shared__ float s_mean[RB_MAX_ATOMS];
  __shared__ float s_ev[RB_MAX_ACTIONS];
  const int i = (int)blockIdx.x;
  rb_head_act_body(Z, A, logits + (int64_t)i * (Z + A * Z), support, s_mean, s_ev, action_out + i, q_out ? q_out + i : nullptr, nullptr,
                   0u, epsilon, rng_seed, rng_round, row0 + i, explored_out ? explored_out + i : nullptr);
}
// n == 1: the one-launch act path has written the greedy (action, q); one wave applies the draw of row `row` on top of it.
// (An action below zero is the act path's error report and stays.)
__global__ __launch_bounds__(64) void k_act_eps_override(int A, float epsilon, uint64_t rng_seed, uint64_t rng_round, int row,
                                                          int32_t* action, uint8_t* explored_out) {
  if (threadIdx.x != 0) return;
  const rb_eps_choice c = rb_eps_draw(rng_seed, rng_round, row, epsilon, A);
  if (c.explore && *action >= 0) *action = c.action;
  if (explored_out) *explored_out = (uint8_t)c.explore;
}
