// learner_internal.h — what the learner's sources share: the parameter layout, the RB_OPTS table, the handle, and the
// declarations of the few host functions that are called across the files (learner.hip is ONE translation unit: the
// headers below are its sections, each included exactly once — several of them define non-template kernels).
#pragma once
#include "conv_fwd.h"
#include "conv_dx.h"
#include "conv_dw.h"
#include "noise_body.h"
#include "adam_body.h"
#include "learner_problems.h"
#include "nl_fwd.h"
#include "nl_bwd.h"
#include "fc_gemm.h"
#include "act_path.h"
#include "rb_common.h"

#include <stdlib.h>

#include <math.h>
#include <string.h>

#include <new>

#define RB_HEAD_MAX_NZ 1408   // 3 logit rows of this many floats live in the head kernel's LDS (18 actions x 51 atoms = 969)
typedef ConvGeom<8, 4, 84, 20> GeomC1;   // model.py:56
typedef ConvGeom<4, 2, 20, 9> GeomC2;    // model.py:57
typedef ConvGeom<3, 1, 9, 7> GeomC3;     // model.py:58
typedef ConvGeom<5, 5, 84, 16> GeomD1;   // model.py:61
typedef ConvGeom<5, 5, 16, 3> GeomD2;    // model.py:62
// geometries of the LAST conv layer of their network (its output is the feature vector of the hidden layer)
#define RB_LAST_CONV_GEOM(G) (G::KS == 3 || (G::KS == 5 && G::IH == 16))


struct ConvLayer {
  int cin, cout, ks, s, ih, oh;
  int K() const { return cin * ks * ks; }
  int P() const { return oh * oh; }
  int IP() const { return ih * ih; }
};

struct Layout {
  int B, Z, A, H, F, NZ, hist, nconv;
  ConvLayer conv[3];
  // offsets (floats) inside the flat parameter buffer
  int64_t conv_w[3], conv_b[3];
  int64_t h_mu, h_sigma, h_bmu, h_bsigma, z_mu, z_sigma, z_bmu, z_bsigma;
  int64_t n_params;
  // offsets inside the flat noise buffer
  int64_t h_ein, h_eout, z_ein, z_eout, n_noise;
};

static int64_t align64(int64_t x) { return (x + 63) / 64 * 64; }

static int make_layout(const rb_learner_config_t* c, Layout* L) {
  RB_REQUIRE(c != nullptr, "learner config is NULL");
  RB_REQUIRE(c->batch >= 1 && c->batch <= 1024, "batch must be in [1,1024]");
  RB_REQUIRE(c->atoms >= 2 && c->atoms <= 256, "atoms must be in [2,256]");
  RB_REQUIRE(c->actions >= 1 && c->actions <= 64, "actions must be in [1,64]");
  RB_REQUIRE(c->atoms * (c->actions + 1) <= RB_HEAD_MAX_NZ, "atoms*(actions+1) must be <= %d (head kernel LDS rows)", RB_HEAD_MAX_NZ);
  RB_REQUIRE(c->history >= 1 && c->history <= 16, "history must be in [1,16]");
  RB_REQUIRE(c->hidden >= 1 && c->hidden <= 8192, "hidden must be in [1,8192]");
  RB_REQUIRE(c->architecture == 0 || c->architecture == 1, "architecture must be 0 (canonical) or 1 (data-efficient)");
  RB_REQUIRE(c->multi_step >= 1, "multi_step must be >= 1");
  RB_REQUIRE(c->v_max > c->v_min, "v_max must exceed v_min");
  memset(L, 0, sizeof(*L));
  L->B = c->batch; L->Z = c->atoms; L->A = c->actions; L->H = c->hidden; L->hist = c->history;
  L->NZ = L->Z + L->A * L->Z;
  if (c->architecture == 0) {
    L->nconv = 3;
    L->conv[0] = ConvLayer{c->history, 32, 8, 4, 84, 20};
    L->conv[1] = ConvLayer{32, 64, 4, 2, 20, 9};
    L->conv[2] = ConvLayer{64, 64, 3, 1, 9, 7};
    L->F = 3136;  // model.py:59
  } else {
    L->nconv = 2;
    L->conv[0] = ConvLayer{c->history, 32, 5, 5, 84, 16};
    L->conv[1] = ConvLayer{32, 64, 5, 5, 16, 3};
    L->F = 576;   // model.py:63
  }
  int64_t off = 0;
  for (int l = 0; l < L->nconv; ++l) {
    L->conv_w[l] = off; off = align64(off + (int64_t)L->conv[l].cout * L->conv[l].K());
    L->conv_b[l] = off; off = align64(off + L->conv[l].cout);
  }
  const int64_t H2 = 2 * L->H;
  L->h_mu = off; off = align64(off + H2 * L->F);
  L->h_sigma = off; off = align64(off + H2 * L->F);
  L->h_bmu = off; off = align64(off + H2);
  L->h_bsigma = off; off = align64(off + H2);
  L->z_mu = off; off = align64(off + (int64_t)L->NZ * L->H);
  L->z_sigma = off; off = align64(off + (int64_t)L->NZ * L->H);
  L->z_bmu = off; off = align64(off + L->NZ);
  L->z_bsigma = off; off = align64(off + L->NZ);
  L->n_params = off;
  int64_t n = 0;
  L->h_ein = n; n = align64(n + 2 * (int64_t)L->F);
  L->h_eout = n; n = align64(n + H2);
  L->z_ein = n; n = align64(n + H2);
  L->z_eout = n; n = align64(n + L->NZ);
  L->n_noise = n;
  return RB_OK;
}


static NetPtrs net_ptrs(const Layout& L, const float* params, const float* noise) {
  NetPtrs p;
  for (int l = 0; l < 3; ++l) {
    p.conv_w[l] = l < L.nconv ? params + L.conv_w[l] : nullptr;
    p.conv_b[l] = l < L.nconv ? params + L.conv_b[l] : nullptr;
  }
  p.h_mu = params + L.h_mu; p.h_sigma = params + L.h_sigma; p.h_bmu = params + L.h_bmu; p.h_bsigma = params + L.h_bsigma;
  p.z_mu = params + L.z_mu; p.z_sigma = params + L.z_sigma; p.z_bmu = params + L.z_bmu; p.z_bsigma = params + L.z_bsigma;
  p.h_ein = noise + L.h_ein; p.h_eout = noise + L.h_eout; p.z_ein = noise + L.z_ein; p.z_eout = noise + L.z_eout;
  return p;
}

// ---------------------------------------------------------------------- RB_OPTS --
// RB_OPTS="key=value,key=value" is the library's ONE tuning / test-hook variable, read when a learner handle is created, never
// per launch.  Every key is a row of this table (DESIGN.md §8 repeats it); rb_learner_create refuses a key that is not, and an
// entry without '=' or without an integer value.
struct RbOpts {
  int generic, fc_gemm, implicit_small, xs, act_fused, spec_draw, spec_stall, img_fast, conv_multi, conv_full, t16, dx_ipb, dw_ipb0, dw_ipb1, dw_ipb2;
};
static const struct { const char* key; int RbOpts::*field; int dflt; const char* what; } rb_opt_table[] = {
  {"generic", &RbOpts::generic, 0, "1: every contraction on the gemm_core.h fallback; 2: the noisy-linear layers only"},
  {"fc_gemm", &RbOpts::fc_gemm, -1, "hidden layer on the LDS-tiled GEMMs of fc_gemm.h: -1 = by shape (from 128 rows per net on), 1 = always, 0 = never"},
  {"implicit_small", &RbOpts::implicit_small, 0, "test hook: RB_LEARNER_IMPLICIT_SIGMA on hidden layers of any size"},
  {"xs", &RbOpts::xs, 0, "row splits of the hidden layer's input gradient: 0 = derived from the hidden size (ceil(2H / 256), at most 4)"},
  {"act_fused", &RbOpts::act_fused, 1, "Agent.act as ONE launch (0: the same kernel, one launch per phase)"},
  {"spec_draw", &RbOpts::spec_draw, 0, "the early draw (opt-in: only append-free loops ever arm it)"},
  {"spec_stall", &RbOpts::spec_stall, 0, "test hook: the early draw's go flag is never stored, the gate in front of the pair expires"},
  {"img_fast", &RbOpts::img_fast, 1, "image-fastest block order of the conv launches (0: the order that image counts off a multiple of 8 get)"},
  {"conv_multi", &RbOpts::conv_multi, -1, "images per workgroup of the conv forward: -1 = by shape (from 256 images on), 0 = one"},
  {"conv_full", &RbOpts::conv_full, 1, "the first layer's whole-image kernel at large batches (0: the chunked kernel)"},
  {"t16", &RbOpts::t16, 1, "the canonical first layer's u8 forward on whole-K 16x16x4 tiles (0: the split-K kernel that history < 4 gets)"},
  {"dx_ipb", &RbOpts::dx_ipb, 0, "images per workgroup of the conv input gradients: 0 = by shape (from batch 64 on)"},
  {"dw_ipb0", &RbOpts::dw_ipb0, 0, "images per workgroup of conv layer 0 in the weight-gradient launch: 0 = by shape"},
  {"dw_ipb1", &RbOpts::dw_ipb1, 0, "... of conv layer 1"},
  {"dw_ipb2", &RbOpts::dw_ipb2, 0, "... of conv layer 2"},
};
static int rb_opts_parse(const char* s, RbOpts* o) {
  for (const auto& row : rb_opt_table) o->*row.field = row.dflt;
  while (s && *s) {
    const char* e = strchr(s, ',');
    const size_t n = e ? (size_t)(e - s) : strlen(s);
    const char* eq = (const char*)memchr(s, '=', n);
    RB_REQUIRE(eq != nullptr && eq > s, "RB_OPTS: entry '%.*s' is not key=value", (int)n, s);
    const size_t kl = (size_t)(eq - s);
    int RbOpts::*field = nullptr;
    for (const auto& row : rb_opt_table)
      if (strlen(row.key) == kl && strncmp(row.key, s, kl) == 0) field = row.field;
    RB_REQUIRE(field != nullptr, "RB_OPTS: unknown key '%.*s'", (int)kl, s);
    char* end = nullptr;
    const long v = strtol(eq + 1, &end, 10);
    RB_REQUIRE(end == s + n && end > eq + 1, "RB_OPTS: key '%.*s' needs an integer value", (int)kl, s);
    o->*field = (int)v;
    s = e ? e + 1 : s + n;
  }
  return RB_OK;
}

// What a configuration allows, and its split counts: derived once by rb_learner_create (learner_plan.h plan_caps)
struct LearnerCaps {
  int fast_fc;          // streamed 16x16x4 noisy-linear kernels usable (alignment preconditions hold)
  int fast_conv;        // LDS-resident conv kernels usable (history <= 4, standard channel counts)
  int hs, xs, ws[3];    // split counts
  int wT[3];            // conv_wT[layer] exists (layers >= 1 of the LDS conv path with cin % 32 == 0)
  int gemm_ws;          // the split-K workspace of k_fc_gemm_fwd exists (gemm_part, gemm_ctr)
};

// ---------------------------------------------------------------------- handle --
struct rb_learner {
  rb_learner_config_t cfg;
  Layout L;
  float *p_online, *p_target, *grads, *n_online, *n_target;   // borrowed
  uint64_t seed;
  uint64_t noise_epoch;
  // owned workspace
  float* act[3];        // [NI][cout][P]; act[nconv-1] doubles as feat [NI][F]
  float* dact[3];       // [B][cout][P]
  float* hpart;         // [hs][NI][2H]
  float* h;             // [NI][2H]
  float *feat_b, *h_b;  // k-blocked copies of feat [NI][F] and h [NI][2H] for the streamed forward kernels
  float *feat_s, *h_s;  // k-blocked SCALED copies for the per-row-noise act path (noisy_rows.h): feat (.) ein_hv | feat (.) ein_ha
                        // [rows_s_cap][2F] and h (.) ein_z [rows_s_cap][2H]; allocated by the first rb_learner_act_batch_rows
  int rows_s_cap;
  float* logits;        // [NI][NZ]
  float* dlogits;       // [B][NZ]
  float* dlogitsT;      // [NZ][B]: the same, transposed (the output layer's input gradient reads its dY operand from it)
  float* dh;            // [B][2H]
  float* dhT;           // [2H][B]: the same, transposed (the hidden layer's input gradient reads its dY operand from it)
  float* dfeat_part;    // [xs][B][F]
  int lazy_dfeat;       // this step: the last conv layer's backward kernels sum the partials themselves (no k_dfeat_finish)
  int lazy_splits;
  RbOpts opt;           // RB_OPTS, read ONCE when the handle is created (rb_opt_table above)
  float* gemm_part;     // split-K partial tiles of k_fc_gemm_fwd: one 64 KB tile per workgroup slot (n_cu of them)
  unsigned* gemm_ctr;   // its per-tile arrival counters (self-resetting)
  float* dw_part[3];    // [ws_l][cout][K+1]
  float* conv_wT[3];    // layers >= 1: the input-gradient kernels' weight operand [S*S phases][cin / 32 tiles][kpad][32], rewritten
                        // every step by tenant workgroups of the head launch (conv_dx.h rb_conv_wt_block); pad rows stay zero
  float* log_ps_a;      // [B][Z]
  float* pns_a;         // [B][Z]
  float* m;             // [B][Z]
  int32_t* a_star;      // [B]
  float* support;       // [Z]
  float* zero_noise;    // [n_noise] zeros (eval mode, model.py:46)
  float* norm_part;     // sum-of-squares partials: [0,1024) k_sumsq; fused producers use [0, norm_slots)
  int norm_conv_base;   // first slot of the conv reduction blocks
  int norm_slots;       // > 0: the last learn() left the gradient's sum of squares in norm_part (no k_sumsq pass needed)
  unsigned long long* noise_ctr;   // [0] Philox epoch of the noise generator, [1] block ticket
  NoiseJob* job_dev;               // [3] device copies of the noise jobs (rb_learner_noise_job), uploaded on request
  unsigned* act_ctr;    // arrival counters of the one-launch act path (act_path.h k_act_fused; monotonic, sharded) + its error word
  unsigned act_epoch;   // launches of k_act_fused so far
  int n_cu;             // compute units of the device (the one-launch act path runs one workgroup per CU)
  int rows_cap;         // image rows the forward buffers (act, hpart, h, feat_b, h_b, logits) hold: 3B, grown by act_batch
  LearnerCaps caps;     // what the configuration allows and its split counts (learner_plan.h plan_caps), derived ONCE at creation
  int dw_slices[3];     // slices actually written by the last conv weight-grad launch of each layer
  ImgSrc cur_src;       // input frames of the learn step in flight
  int sink_done;        // the last learn() performed the priority write-back itself
  const int32_t* batch_status;   // device word (the sink replay's header.last_status): non-zero = the sampler gave up on the
                                 // batch in flight; the optimiser update and its step number are then skipped (k_head, k_clip_adam)
  rb_replay_t* sink;    // priority sink: when set, learn() writes loss^w back into this replay's sum-tree itself
  const int64_t* sink_idx;
  // replica exchange: world > 1 defers the noisy-linear WEIGHT gradients — instead of all-reducing 27 MB of
  // gradient, the replicas all-gather the two factors of every FC gradient (dY and X rows, 0.7 MB per rank) and each
  // computes the replica-mean gradient from the gathered rows itself (rb_learner_finish_grads)
  int world;
  float* fact_local;        // [fact_stride] this rank's factor block, written by the learn call
  const float* fact_all;    // [world][fact_stride] every rank's block (the all-gather's output)
  int64_t fact_off[6];      // dlogits [B][NZ] | h [B][2H] | dh [B][2H] | feat [B][F] | this rank's online noise [n_noise] |
                            // this rank's conv gradients (the leading h_mu floats of the flat gradient)
  int64_t fact_stride;
  int exch_pending;         // a learn call left its FC weight gradients to rb_learner_finish_grads
  long long* step_ctr;      // optional device-resident optimiser step counter (rb_learner_set_step_counter)
  int flags;                // RB_LEARNER_FUSE_FC_H_DW | RB_LEARNER_WRITE_FUSED_GRADS (rb_learner_set_flags)
  int dw_deferred;          // the last learn call computed the hidden layer's weight gradient for its norm only: the
                            // optimiser pass (rb_learner_clip_adam) recomputes the tiles while it streams the parameters
  // RB_LEARNER_DEFER_UPDATE: rb_learner_train_step leaves its optimiser pass PENDING; the next train_step's sampler launch
  // hosts it as extra workgroups (adam_body.h), every other entry point that touches parameters, moments, gradients or
  // the norm runs it first as a launch of its own (flush_update)
  ClipAdamArgs* adam_args_dev;   // the pending pass's arguments in device memory (rewritten only when they change)
  ClipAdamArgs adam_args_host;   // ... and what that memory holds
  int adam_args_valid, adam_pending, adam_blocks;
  float target_tau;              // rb_learner_set_target_tau: > 0 = every optimiser pass moves p_target by this EMA (0: off)
  // The early draw (RB_OPTS spec_draw=1, OFF by default; replay_internal.h rb_replay_spec_launch): from the second back-to-back
  // rb_learner_train_step on the same replay with nothing in between, the priority write-back leaves the hidden layer's backward
  // launch and runs — together with the NEXT call's draw — on the replay's own stream as soon as the head kernel is done; the next
  // call's sampler launch accepts the draw and carries only the noise and the pending optimiser pass.  Only an append-free,
  // constant-beta loop ever arms it (a PER benchmark; never main.py's loop), every wait is bounded at ~2 ms and fails safe, and the
  // first expiry disables it on the handle.  RB_OPTS spec_stall=1 (test hook): the launch behind the head kernel does
  // not store the go flag — the gate in front of the pair expires.
  // (A SPLIT optimiser pass — the (mu, sigma) pair workgroups on a second stream beside the sampler and the conv forward, the hidden
  // layer's forward waiting in-kernel for their arrival — was built in round 5, bit-identical, and measured 177 us per step against
  // 161.5: profiles/round5_split_experiments.txt; removed, the code is commit 645f60a.)
  unsigned* go_flag;          // device word: epoch of the last head kernel known complete (stored by the launch behind it)
  unsigned go_epoch;
  int spec_now;               // this train_step: the write-back and the next draw go to the replay's stream
  rb_spec_request spec_req;
  struct { rb_replay_t* replay; int32_t batch, max_attempts; double beta; int64_t* tree_idx; int64_t* actions; float* returns; float* nonterm;
           float* weights; unsigned long long mut_after; int valid, streak; } ts_last;
  // RB_LEARNER_IMPLICIT_SIGMA: the hidden layer's sigma-weight gradient is not stored by the backward; the hosted optimiser
  // pass forms it from g_mu and the noise the backward used (adam_body.h rb_adam_hosted_pairs).  sigma_implicit = the flat
  // gradient lacks that range right now; every other consumer of the gradient materialises it first (materialize_sigma)
  int sigma_implicit;
  float* noise_snap;        // [n_noise] the online noise of the learn call in flight, copied by its last backward launch
  int32_t* status_copy;     // this learn call's batch_status, copied by its head kernel: the hosted pass shares a launch with
                            // the NEXT call's sampler, which overwrites the replay header's word
  float gamma_n;        // float32(discount ** n)        agent.py:79  (n and discount: the two below)
  int32_t n_eff;        // the effective horizon (rb_learner_set_horizon; cfg.multi_step until then): the next-state slot of the window
  double discount;      // table (SrcDesc n_step) and the exponent of gamma_n — host state, read when a step is launched
  float delta_z;        // float32((Vmax - Vmin)/(Z-1))   agent.py:19,82
  // device-side read-outs (learn_stats.h): the caller's record ring (rb_learner_set_stats; NULL = off, no launch) and the scratch
  // k_step_stats and rb_learner_eval_loss need, allocated by the first of them that is used
  rb_step_stats_t* stats_ring;
  long long* stats_count;
  int stats_cap;
  double* stats_rows;       // [3][B] per-row q, q_target, entropy
  unsigned* stats_ticket;   // arrival counter of k_step_stats (self-resetting)
  float* ones;              // [B] unit importance weights of rb_learner_eval_loss
};

// ---- host functions called across the learner's files
// optimizer_host.h: the pending optimiser pass (RB_LEARNER_DEFER_UPDATE) as a launch of its own; the hidden layer's sigma
// gradient that RB_LEARNER_IMPLICIT_SIGMA's backward left out
static int flush_update(rb_learner* l, hipStream_t stream);
static int materialize_sigma(rb_learner* l, hipStream_t stream);
// rb_comm.hip: the communicator behind rb_learner_exchange_rccl (an all-gather of `count` floats per rank on `stream`)
int rb_comm_world(const rb_comm_t* comm);
int rb_comm_all_gather_f32(rb_comm_t* comm, const float* send, float* recv, size_t count, hipStream_t stream);

#define RB_FLUSH_UPDATE(l, stream)                                  \
  do {                                                              \
    const int rcf_ = flush_update((l), (hipStream_t)(stream));      \
    if (rcf_ != RB_OK) return rcf_;                                 \
  } while (0)
#define RB_MATERIALIZE_SIGMA(l, stream)                             \
  do {                                                              \
    const int rcm_ = materialize_sigma((l), (hipStream_t)(stream)); \
    if (rcm_ != RB_OK) return rcm_;                                 \
  } while (0)
