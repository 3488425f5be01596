// act_path.h — Agent.act / evaluate_q (agent.py:53-55, 110-112; main.py:153, test.py:26,39): the forward of ONE un-batched state
// and its head as a persistent launch, k_act_fused, over the bodies of act_conv.h (one output channel or one MFMA tile per unit),
// act_fc.h (one weight row per wave) and act_head.h.  Included by learner_internal.h; launched by act_host.h act_forward_single.
//
// The forward is six phases {conv 0, 1, 2, fc_h, fc_z, head}; phase_lo / phase_hi: a launch runs phases [lo, hi).  As six launches
// it took 59 us for 22 MFLOP and 27 MB, half of main.py's loop period once a learn step is 170 us.  ONE launch with all six is the
// product path: G workgroups (one per CU) walk the phases together; a phase boundary is an all-to-all hand-off: every workgroup
// stores its outputs write-through, arrives on the boundary's counter, polls it and reads the previous layer with agent-coherent
// loads (rb_device.h rb_chain_*: the form validated for in-launch hand-offs).  What does NOT depend on the previous layer is
// requested before the wait: the hidden layer's 25.7 MB of mu | sigma — the bulk of the forward's bytes — stream into REGISTERS
// (one weight row per wave) while the conv phases run, so that phase is one small activation load + FMAs.
// Counters are monotonic (target = launch number x G): no reset between launches.  Every spin is bounded; on expiry the
// error word is set and the head writes action -1.
// A launch of ONE phase has no in-launch dependency — it prefetches nothing, waits for nothing and signals nothing — and runs
// the same units in the same order: six of them are the other launch form (RB_OPTS act_fused=0, stream capture, the host
// interpreter; act_host.h has the conditions), with the one launch's arithmetic and summation order, bit for bit.
#pragma once
#include "act_conv.h"
#include "act_fc.h"
#include "act_head.h"
#include "kernel_stamp.h"

struct ActFusedArgs {
  ActConvArgs conv[3];
  int nconv;
  ActFcArgs h, z;
  int Z, A;
  const float* logits;     // = z.out
  const float* support;
  int32_t* action_out;
  float* q_out;
  unsigned* ctr;           // [6][8 shards x 32 words] arrival counters, one set per phase (rb_device.h rb_fan_*)
  unsigned epoch;
  unsigned* err;
  int phase_lo, phase_hi;
};

// HQ: quads of a hidden-layer weight row per lane kept in registers across the conv phases (ceil(F / 256): 13 canonical, 3
// data-efficient; 0 = no prefetch, any shape).  grid = G workgroups (all resident: G <= CUs), block = 256.
template <int HQ>
__global__ __launch_bounds__(256) void k_act_fused(ActFusedArgs a) {
  __shared__ __attribute__((aligned(16))) float s_in[RB_ACT_LDS];
  __shared__ float s_red[4][RB_ACT_MAXPOS];
  __shared__ float s_w[RB_ACT_KMAX];
  const int wg = (int)blockIdx.x, G = (int)gridDim.x;
  const int t = (int)threadIdx.x;
  const int wave = rb_wave_uniform(t >> 6);
  const bool fused = a.phase_hi - a.phase_lo > 1;
  float4 hm[HQ > 0 ? HQ : 1], hs[HQ > 0 ? HQ : 1];
  // the hidden layer's row of this wave, requested first thing by every workgroup (requesting it AFTER the first layer's unit
  // in the workgroups that have one measured slower: 35.5 against 33.3 us for the launch)
  if (HQ > 0 && fused && a.phase_lo <= 3 && a.phase_hi > 3) rb_act_fc_prefetch<HQ>(a.h, 4 * wg + wave, hm, hs);
  int prev = -1, prev_units = 0;
  RB_WGT(10, wg, 0);                                             // RB_STAMP builds: slot 0 start, slot 1 + phase = end of that phase
  RB_WGT(11, wg, 0);                                             // ... kernel id 11: slot 1 + phase = the phase's wait is over
  for (int phase = a.phase_lo; phase < a.phase_hi; ++phase) {
    if (phase < 3 && phase >= a.nconv) continue;                 // (two conv layers: phase 2 does not exist)
    // units of work of the phase (workgroup wg takes units wg, wg + G, ...: it has work iff wg < units); tiles > 0: a conv layer
    // whose units are MFMA tiles
    int tiles = 0, units = 1;                                    // (the head is one unit)
    if (phase < 3) {
      const ActConvArgs& c = a.conv[phase];
      tiles = rb_act_conv_tiles(c);
      units = tiles > 0 ? tiles : c.cout * ((c.OH + c.RG - 1) / c.RG);
    } else if (phase < 5) {
      units = ((phase == 3 ? a.h.n_rows : a.z.n_rows) + 3) / 4;
    }
    // Only the workgroups WITH work in a phase arrive at its boundary, and only those with work in the next one wait for it
    // (round 6: the conv phases have 50 / 24 / 16 units, the output layer 90 — with every one of the 256 workgroups arriving and
    // polling at every boundary, ~200 idle pollers sat on the counter lines the few working workgroups had to get their arrivals
    // through).  Transitive: a producer of boundary p waited for boundary p - 1 before it produced.
    const bool has_work = wg < units;                            // block-uniform
    if (prev >= 0 && has_work)
      rb_fan_wait_first(a.ctr + prev * (RB_FAN_SHARDS * RB_FAN_STRIDE), a.epoch, prev_units < G ? prev_units : G, a.err, a.epoch);
    RB_WGT(11, wg, 1 + phase);
    if (phase < 3) {
      const ActConvArgs& c = a.conv[phase];
      if (tiles > 0) {
        for (int u = wg; u < units; u += G) rb_act_conv_tile_any(c, u, s_in);
      } else {
        for (int u = wg; u < units; u += G) rb_act_conv_unit(c, u % c.cout, (u / c.cout) * c.RG, s_in, s_red, s_w);
      }
    } else if (phase == 3) {
      for (int u = wg; u < units; u += G) {
        const int row = 4 * u + wave;
        if (row < a.h.n_rows) {
          if (HQ > 0 && fused && u == wg) rb_act_fc_row<HQ>(a.h, row, hm, hs);
          else rb_act_fc_row<0>(a.h, row, nullptr, nullptr);
        }
      }
    } else if (phase == 4) {
      for (int u = wg; u < units; u += G) {
        const int row = 4 * u + wave;
        if (row < a.z.n_rows) rb_act_fc_row<0>(a.z, row, nullptr, nullptr);
      }
    } else if (has_work) {
      // head (k_head_act's arithmetic) on the logits staged in LDS through coherent loads
      const int NZ = a.Z + a.A * a.Z;
      const rb_buf bl = rb_make_buf(a.logits);
      float* lg = s_in;                                            // NZ <= RB_HEAD_MAX_NZ <= RB_ACT_LDS
      for (int i = t; i < NZ; i += 256) lg[i] = rb_ld1_buf_sc1(bl, 4u * (unsigned)i, 0u);
      float* s_mean = s_w;                                         // Z <= 256 <= RB_ACT_KMAX
      float* s_ev = &s_red[0][0];                                  // A <= 64
      __syncthreads();
      rb_head_act_body(a.Z, a.A, lg, a.support, s_mean, s_ev, a.action_out, a.q_out, a.err, a.epoch);
    }
    RB_WGT(10, wg, 1 + phase);
    if (phase + 1 < a.phase_hi && has_work) rb_fan_signal(a.ctr + phase * (RB_FAN_SHARDS * RB_FAN_STRIDE), wg);
    prev = phase; prev_units = units;
  }
}
