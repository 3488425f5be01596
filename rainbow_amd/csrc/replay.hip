// replay.hip — HBM-resident prioritised replay for MI355X (gfx950).
//
// What it replaces: the host-RAM numpy SegmentTree/ReplayMemory of the reference
// (memory.py:12-180).  Layout here is SoA in HBM (frames u8[C][7056] + 4 small
// columns) with the reference's level-order float32 sum-tree (same truncated leaf
// level, memory.py:17-18) so tree indices are interchangeable with the reference's.
//
// Invariant used everywhere: every internal node equals fl32(left + right) of its
// CURRENT children (memory.py:25,39), i.e. the tree is a pure function of its leaves.
// Batched updates therefore rebuild ancestors level by level and land on exactly the
// floats the reference's sequential walks produce.
//
// All of this is HBM-latency / HBM-bandwidth work (no GEMM shape anywhere): the frame
// gather moves (h+n)·7056 B in and 2h·7056 B out per sample with 16-byte lanes, the tree
// search is L dependent 4-byte loads per sample.
#include "noise_body.h"
#include "adam_body.h"
#include "replay_internal.h"
#include "replay_search.h"
#include "replay_append.h"
#include "replay_spec.h"
#include "replay_sample.h"
#include "replay_shift.h"
#include "replay_view.h"
#include "replay_stats.h"

#include <stdlib.h>
#include <string.h>

#include <new>

// ---------------------------------------------------------------------- handle --
struct rb_replay {
  int64_t capacity;
  int32_t history, n;   // n = n_max, the multi_step of creation: every allocation, the window table's row stride history + n
  int32_t n_eff;        // the effective horizon, 1 <= n_eff <= n (rb_replay_set_horizon; n until then)
  double discount;      // the discount scaling[] was last filled from
  int32_t levels;       // L = depth of the leaf level
  int32_t streams;      // S interleaved environment streams (1 = the reference's single sequential stream)
  int64_t tree_start;   // 2^L - 1
  int64_t tree_len;     // tree_start + capacity
  double omega;         // priority exponent (memory.py:99)
  uint64_t seed;
  float scaling[64];    // gamma^k as float32(double pow)  (memory.py:101)
  // device
  float* tree;
  uint8_t* frames;
  int32_t* timestep;
  int32_t* action;
  float* reward;
  uint8_t* nonterminal;
  rb_replay_header_t* hdr;
  int32_t* win;         // [max_batch][h+n] ring index of each window slot, -1 = blank
  float* scaling_dev;
  int32_t max_batch;
  const float* neg_beta_dev;   // optional device-resident -beta (graph replay: no by-value argument may change)
  int32_t* fail_host;          // pinned, device-mapped, four words: [0] sampler launches that found no valid batch (see k_sample),
                               // [1] priority write-backs dropped because their indices came from such a draw (rb_update_body),
                               // [2] expired cross-stream waits of the early draw (rb_poll_epoch; must stay 0)
  // host mirror of the deterministic part of the header
  int64_t host_index;
  int32_t host_full;
  // the early draw (replay_internal.h rb_replay_spec_launch)
  int32_t* win2;               // the second window table
  int win_sel;                 // table of the last draw (0 = win, 1 = win2)
  hipStream_t spec_stream;
  SpecResult* spec_res;        // device
  unsigned spec_epoch;
  int spec_inflight;
  struct { int32_t batch, max_attempts, win_set; double beta; int64_t* tree_idx; int64_t* actions; float* returns; float* nonterm; float* weights; } spec_args;
  unsigned long long mutations;   // entry points that changed the replay (or drew from it) so far
  int spec_accept_armed;          // the NEXT draw on the handle may accept a tentative draw (set by rb_learner_train_step only, one shot:
                                  // the public sample entry points always redraw into table 0 = rb_replay_buffers_t.window_dev)
  int spec_disabled;              // an expired cross-stream wait was seen (fail_host[2]): no early draw on this handle until
                                  // rb_replay_reset_failed_samples
  PriorityScratch* pstats;        // per-workgroup partials of rb_replay_priority_stats (replay_stats.h), allocated by its first call
};
static int32_t* win_of(const rb_replay* r, int set) { return set ? r->win2 : r->win; }
// every entry point that reads or writes the replay outside a draw: wait for an early draw in flight and discard it (its
// write-back part is final and stays, its tentative draw is simply never accepted)
static int spec_join(rb_replay* r) {
  if (!r->spec_inflight) return RB_OK;
#if !defined(RB_HOST_INTERP)
  RB_HIP_TRY(hipStreamSynchronize(r->spec_stream));
#endif
  r->spec_inflight = 0;
  return RB_OK;
}
#define RB_SPEC_JOIN(r)                 \
  do {                                  \
    const int rcj_ = spec_join(r);      \
    if (rcj_ != RB_OK) return rcj_;     \
  } while (0)

static ReplayView view_of(const rb_replay* r) {
  ReplayView v;
  v.capacity = r->capacity; v.history = r->history; v.n = r->n_eff; v.levels = r->levels; v.streams = r->streams;
  v.tree_start = r->tree_start; v.tree_len = r->tree_len;
  v.tree = r->tree; v.frames = r->frames; v.timestep = r->timestep; v.action = r->action;
  v.reward = r->reward; v.nonterminal = r->nonterminal; v.hdr = r->hdr;
  v.dropped = r->fail_host ? r->fail_host + 1 : nullptr;
  return v;
}

// Live handles, so that a raw header restore through rb_copy_to_device (state load, main.py:118) refreshes the host
// mirror of index/full that rb_replay_append_batch plans its ancestor rebuild from.
static rb_replay* g_live[64];
static void live_add(rb_replay* r) { for (auto& p : g_live) if (!p) { p = r; return; } }
static void live_del(rb_replay* r) { for (auto& p : g_live) if (p == r) p = nullptr; }
void rb_replay_note_device_write(void* dst_dev, const void* src_host, size_t nbytes) {
  for (rb_replay* r : g_live) {
    if (!r || !r->hdr) continue;
    const char* h = (const char*)r->hdr;
    const char* d = (const char*)dst_dev;
    if (d <= h && h + sizeof(rb_replay_header_t) <= d + nbytes) {
      rb_replay_header_t hd;
      memcpy(&hd, (const char*)src_host + (h - d), sizeof(hd));
      r->host_index = hd.index;
      r->host_full = hd.full;
    }
  }
}

// ---------------------------------------------------- the early draw, host side --
// (interface: replay_internal.h; protocol and device side: replay_spec.h; the accepting end: sample_impl)
int rb_replay_spec_inflight(rb_replay_t* r) { return r ? r->spec_inflight : 0; }
const int32_t* rb_replay_current_windows(rb_replay_t* r) { return win_of(r, r->win_sel); }
unsigned long long rb_replay_mutations(rb_replay_t* r) { return r->mutations; }
void rb_replay_horizon(rb_replay_t* r, int32_t* n_eff, double* discount) { *n_eff = r->n_eff; *discount = r->discount; }

// (replay_internal.h) the write-back of learn call k + the tentative draw of call k + 1 on the replay's own stream
int rb_replay_spec_allowed(rb_replay_t* r) {
  if (!r) return 0;
  if (*(volatile int32_t*)(r->fail_host + 2) != 0) r->spec_disabled = 1;   // an expired wait: the handle stays without early draws
  return r->spec_disabled ? 0 : 1;
}
void rb_replay_spec_arm_accept(rb_replay_t* r) { r->spec_accept_armed = 1; }

int rb_replay_spec_launch(rb_replay_t* r, const rb_spec_request& q) {
  RB_REQUIRE(r && q.upd_idx && q.upd_loss && q.tree_idx && q.actions && q.returns && q.nonterminals && q.weights, "rb_replay_spec_launch: NULL argument");
  RB_REQUIRE(q.batch >= 1 && q.batch <= 256 && q.upd_n >= 1 && q.upd_n <= 256, "rb_replay_spec_launch: batch and upd_n must be in [1,256]");
  RB_REQUIRE(r->capacity > (int64_t)r->history + r->n, "rb_replay_spec_launch: capacity must exceed history + multi_step");
  RB_SPEC_JOIN(r);
#if defined(RB_HOST_INTERP)
  hipStream_t s2 = nullptr;
#else
  if (!r->spec_stream) RB_HIP_TRY(hipStreamCreateWithFlags(&r->spec_stream, hipStreamNonBlocking));
  hipStream_t s2 = r->spec_stream;
#endif
  const ReplayView v = view_of(r);
  const int win_set = r->win_sel ^ 1;            // the table the step in flight still reads is left alone
  const float neg_beta = (float)(-q.priority_weight);
  const unsigned epoch = ++r->spec_epoch;
  ++r->mutations;
  if (q.go_flag) {
    RB_LAUNCH(k_spec_gate, dim3(1), dim3(64), s2, q.go_flag, q.go_epoch, r->fail_host + 2, r->spec_res, epoch);
    RB_LAUNCH_CHECK();
  }
  // one launch (latency is no concern on this stream): sorted batches of up to 64 leaves take the one-wave write-back, the rest
  // the hashed body inside the same kernel
  RB_LAUNCH(k_update_sample, dim3(1), dim3(256), s2, v, q.upd_idx, q.upd_loss, q.upd_n, 1, r->omega, q.batch, neg_beta, r->neg_beta_dev,
            (const double*)nullptr, q.max_attempts, r->seed, r->scaling_dev, q.tree_idx, win_of(r, win_set), q.actions, q.returns,
            q.nonterminals, q.weights, r->fail_host, r->spec_res, epoch);
  RB_LAUNCH_CHECK();
  r->spec_args.batch = q.batch; r->spec_args.max_attempts = q.max_attempts; r->spec_args.win_set = win_set;
  r->spec_args.beta = q.priority_weight; r->spec_args.tree_idx = q.tree_idx; r->spec_args.actions = q.actions;
  r->spec_args.returns = q.returns; r->spec_args.nonterm = q.nonterminals; r->spec_args.weights = q.weights;
  r->spec_inflight = 1;
  return RB_OK;
}

int rb_replay_internal_view(rb_replay_t* r, ReplayView* view, double* omega) {
  if (!r || !view || !omega) return RB_ERR_INVALID;
  *view = view_of(r);
  *omega = r->omega;
  return RB_OK;
}

// ================================================================ C ABI entry points
// ------------------------------------------------------------------- lifecycle --
__global__ void k_replay_init(rb_replay_header_t* hdr) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    hdr->index = 0;
    hdr->full = 0;
    hdr->max = 1.0f;  // memory.py:20  (1 = 1^w)
    hdr->total = 0.0f;
    hdr->last_attempts = 0;
    hdr->last_status = 0;
    hdr->rng_counter = 0;
  }
}

// gamma^k for rb_replay_set_horizon: the table travels BY VALUE in the kernel arguments and is stored in stream order — a sampler
// launch queued before this one reads the old table, the next one the new, with no copy from pageable memory and no synchronisation
struct HorizonTable { float s[64]; };
__global__ __launch_bounds__(64) void k_set_horizon(float* scaling, HorizonTable tab) {
  const int t = (int)threadIdx.x;
  if (blockIdx.x == 0 && t < 64) scaling[t] = tab.s[t];
}

extern "C" {

static int create_impl(rb_replay_t** out, int64_t capacity, int32_t history, int32_t multi_step, double discount,
                       double priority_exponent, uint64_t seed, int32_t streams) {
  RB_REQUIRE(out != nullptr, "rb_replay_create: out is NULL");
  RB_REQUIRE(capacity >= 2 && (capacity % 2) == 0,
             "rb_replay_create: capacity must be even and >= 2 (the reference's sum-tree walk reads past the "
             "array for odd sizes, memory.py:38-39), got %lld", (long long)capacity);
  RB_REQUIRE(capacity <= ((int64_t)1 << 30), "rb_replay_create: capacity too large");
  RB_REQUIRE(history >= 1 && multi_step >= 1 && history + multi_step <= 64, "rb_replay_create: need history>=1, multi_step>=1, history+multi_step<=64");
  rb_replay* r = new (std::nothrow) rb_replay();
  if (!r) { rb_set_error("rb_replay_create: host OOM"); return RB_ERR_OOM; }
  r->capacity = capacity; r->history = history; r->n = multi_step; r->omega = priority_exponent; r->seed = seed;
  r->streams = streams; r->n_eff = multi_step; r->discount = discount;
  int32_t L = 0;
  while (((int64_t)1 << L) < capacity) ++L;  // (capacity-1).bit_length()   memory.py:17
  r->levels = L;
  r->tree_start = ((int64_t)1 << L) - 1;
  r->tree_len = r->tree_start + capacity;
  for (int k = 0; k < multi_step; ++k) r->scaling[k] = (float)pow(discount, (double)k);  // memory.py:101
  { const int32_t stride = history + multi_step; memcpy(&r->scaling[RB_STRIDE_SLOT], &stride, sizeof(stride)); }   // replay_internal.h
  r->max_batch = 1024;            // (every other field stays as rb_replay() value-initialised it: null, 0)
#define RB_ALLOC(ptr, bytes)                                                                      \
  do {                                                                                            \
    hipError_t e_ = rb_dev_malloc((void**)&(ptr), (size_t)(bytes));                                   \
    if (e_ != hipSuccess) {                                                                       \
      rb_set_error("rb_replay_create: hipMalloc(%lld B) failed: %s", (long long)(bytes), hipGetErrorString(e_)); \
      rb_replay_destroy(r);                                                                       \
      return RB_ERR_OOM;                                                                          \
    }                                                                                             \
  } while (0)
  RB_ALLOC(r->tree, (r->tree_len + RB_TREE_PAD) * sizeof(float));
  RB_ALLOC(r->frames, capacity * (int64_t)RB_FRAME_BYTES);
  RB_ALLOC(r->timestep, capacity * sizeof(int32_t));
  RB_ALLOC(r->action, capacity * sizeof(int32_t));
  RB_ALLOC(r->reward, capacity * sizeof(float));
  RB_ALLOC(r->nonterminal, capacity);
  RB_ALLOC(r->hdr, sizeof(rb_replay_header_t));
  RB_ALLOC(r->win, (int64_t)r->max_batch * 64 * sizeof(int32_t));
  RB_ALLOC(r->win2, (int64_t)r->max_batch * 64 * sizeof(int32_t));
  RB_ALLOC(r->spec_res, sizeof(SpecResult));
  RB_ALLOC(r->scaling_dev, 64 * sizeof(float));
#undef RB_ALLOC
  {
    hipError_t e_ = hipHostMalloc((void**)&r->fail_host, 4 * sizeof(int32_t), hipHostMallocMapped);
    if (e_ != hipSuccess) {
      rb_set_error("rb_replay_create: hipHostMalloc failed: %s", hipGetErrorString(e_));
      rb_replay_destroy(r);
      return RB_ERR_OOM;
    }
    r->fail_host[0] = 0; r->fail_host[1] = 0; r->fail_host[2] = 0; r->fail_host[3] = 0;
  }
  // blank_trans everywhere (memory.py:8,19), zero tree (memory.py:18)
  RB_HIP_TRY(hipMemset(r->tree, 0, (r->tree_len + RB_TREE_PAD) * sizeof(float)));
  RB_HIP_TRY(hipMemset(r->frames, 0, capacity * (int64_t)RB_FRAME_BYTES));
  RB_HIP_TRY(hipMemset(r->timestep, 0, capacity * sizeof(int32_t)));
  RB_HIP_TRY(hipMemset(r->action, 0, capacity * sizeof(int32_t)));
  RB_HIP_TRY(hipMemset(r->reward, 0, capacity * sizeof(float)));
  RB_HIP_TRY(hipMemset(r->nonterminal, 0, capacity));
  RB_HIP_TRY(hipMemcpy(r->scaling_dev, r->scaling, 64 * sizeof(float), hipMemcpyHostToDevice));
  RB_HIP_TRY(hipMemset(r->spec_res, 0, sizeof(SpecResult)));
  RB_LAUNCH(k_replay_init, dim3(1), dim3(64), nullptr, r->hdr);
  RB_LAUNCH_CHECK();
  RB_HIP_TRY(hipDeviceSynchronize());
  live_add(r);
  *out = r;
  return RB_OK;
}

int rb_replay_create(rb_replay_t** out, int64_t capacity, int32_t history, int32_t multi_step, double discount,
                     double priority_exponent, uint64_t seed) {
  return create_impl(out, capacity, history, multi_step, discount, priority_exponent, seed, 1);
}

int rb_replay_create_streams(rb_replay_t** out, int64_t capacity, int32_t history, int32_t multi_step, double discount,
                             double priority_exponent, uint64_t seed, int32_t streams) {
  if (out) *out = nullptr;
  RB_REQUIRE(streams >= 1 && streams <= RB_MAX_STREAMS, "rb_replay_create_streams: streams must be in [1, %d], got %d",
             RB_MAX_STREAMS, (int)streams);
  RB_REQUIRE(capacity % streams == 0, "rb_replay_create_streams: capacity %lld is not a multiple of streams %d (a round of "
             "appends must never wrap)", (long long)capacity, (int)streams);
  RB_REQUIRE(history < 1 || multi_step < 1 || capacity > (int64_t)(history + multi_step) * streams,
             "rb_replay_create_streams: capacity %lld must exceed (history + multi_step) * streams = %lld (every stream's window "
             "must fit its share of the ring)", (long long)capacity, (long long)(history + multi_step) * streams);
  return create_impl(out, capacity, history, multi_step, discount, priority_exponent, seed, streams);
}

int rb_replay_destroy(rb_replay_t* r) {
  if (!r) return RB_OK;
  (void)spec_join(r);
#if !defined(RB_HOST_INTERP)
  if (r->spec_stream) (void)hipStreamDestroy(r->spec_stream);
#endif
  live_del(r);
  if (r->pstats) rb_dev_free(r->pstats);
  if (r->win2) rb_dev_free(r->win2);
  if (r->spec_res) rb_dev_free(r->spec_res);
  if (r->tree) rb_dev_free(r->tree);
  if (r->frames) rb_dev_free(r->frames);
  if (r->timestep) rb_dev_free(r->timestep);
  if (r->action) rb_dev_free(r->action);
  if (r->reward) rb_dev_free(r->reward);
  if (r->nonterminal) rb_dev_free(r->nonterminal);
  if (r->hdr) rb_dev_free(r->hdr);
  if (r->win) rb_dev_free(r->win);
  if (r->scaling_dev) rb_dev_free(r->scaling_dev);
  if (r->fail_host) (void)hipHostFree(r->fail_host);
  delete r;
  return RB_OK;
}

int rb_replay_buffers(rb_replay_t* r, rb_replay_buffers_t* o) {
  RB_REQUIRE(r && o, "rb_replay_buffers: NULL argument");
  RB_SPEC_JOIN(r);
  o->sum_tree_dev = r->tree; o->tree_len = r->tree_len; o->tree_start = r->tree_start;
  o->frames_dev = r->frames; o->timestep_dev = r->timestep; o->action_dev = r->action;
  o->reward_dev = r->reward; o->nonterminal_dev = r->nonterminal; o->header_dev = r->hdr;
  o->window_dev = r->win; o->window_len = r->history + r->n;
  return RB_OK;
}

int rb_replay_header(rb_replay_t* r, rb_replay_header_t* o, rb_stream_t stream) {
  RB_REQUIRE(r && o, "rb_replay_header: NULL argument");
  RB_SPEC_JOIN(r);
  RB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  RB_HIP_TRY(hipMemcpy(o, r->hdr, sizeof(*o), hipMemcpyDeviceToHost));
  r->host_index = o->index;  // resynchronise the mirror (e.g. after a state restore)
  r->host_full = o->full;
  return RB_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------ append --
// One round of S streams (k_append_streams), whichever way its per-stream operands come: `ops` is the kernel's operand block, NULL
// when the entry point `entry` was handed a NULL operand array.
template <class Ops>
static int append_round(rb_replay* r, const char* entry, const char* tag, const float* states_dev, const Ops* ops, rb_stream_t stream) {
  RB_REQUIRE(r && states_dev && ops, "%s: NULL argument", entry);
  RB_REQUIRE(((uintptr_t)states_dev & 15u) == 0, "%s: states_dev must be 16-byte aligned", entry);
  const int S = r->streams;
  RB_REQUIRE(r->host_index % S == 0, "%s: the write head (%lld) is not at a round boundary of %d streams", entry,
             (long long)r->host_index, S);
  RB_SPEC_JOIN(r);
  ++r->mutations;
  const int64_t start = r->host_index;
  RB_LAUNCH_T(tag, k_append_streams<Ops>, dim3((unsigned)S + 1u), dim3(256), stream, view_of(r), states_dev, start, *ops);
  RB_LAUNCH_CHECK();
  r->host_index = (start + S) % r->capacity;
  if (r->host_index == 0) r->host_full = 1;
  return RB_OK;
}

extern "C" {

int rb_replay_append(rb_replay_t* r, const float* state_dev, int32_t timestep, int32_t action, float reward,
                     int32_t nonterminal, rb_stream_t stream) {
  RB_REQUIRE(r && state_dev, "rb_replay_append: NULL argument");
  RB_REQUIRE(r->streams == 1, "rb_replay_append: this replay holds %d interleaved streams: append whole rounds with "
             "rb_replay_append_streams", (int)r->streams);
  RB_SPEC_JOIN(r);
  ++r->mutations;
  const float* last = state_dev + (int64_t)(r->history - 1) * RB_FRAME_BYTES;  // state[-1], memory.py:106
  RB_LAUNCH(k_append_one, dim3(1), dim3(256), stream, view_of(r), last, timestep, action, reward, nonterminal);
  RB_LAUNCH_CHECK();
  r->host_index = (r->host_index + 1) % r->capacity;
  if (r->host_index == 0) r->host_full = 1;
  return RB_OK;
}

int rb_replay_append_batch(rb_replay_t* r, const uint8_t* frames_dev, const int32_t* timesteps_dev,
                           const int32_t* actions_dev, const float* rewards_dev, const uint8_t* nonterminals_dev,
                           int64_t n, rb_stream_t stream) {
  RB_REQUIRE(r && frames_dev && timesteps_dev && actions_dev && rewards_dev && nonterminals_dev,
             "rb_replay_append_batch: NULL argument");
  RB_SPEC_JOIN(r);
  ++r->mutations;
  RB_REQUIRE(n >= 0 && n <= r->capacity, "rb_replay_append_batch: n must be in [0, capacity]");
  RB_REQUIRE(n % r->streams == 0 && r->host_index % r->streams == 0, "rb_replay_append_batch: with %d interleaved streams n "
             "must be whole rounds (a multiple of the stream count) and the write head at a round boundary", (int)r->streams);
  if (n == 0) return RB_OK;
  const ReplayView v = view_of(r);
  const int64_t start = r->host_index;
  const int grid = (int)(n < 4096 ? n : 4096);
  RB_LAUNCH(k_append_copy, dim3(grid), dim3(256), stream, v, start, frames_dev, timesteps_dev, actions_dev,
            rewards_dev, nonterminals_dev, n);
  RB_LAUNCH_CHECK();
  // leaf ranges (tree indices), possibly wrapping around the ring
  int64_t lo0 = r->tree_start + start, hi0, lo1 = 0, hi1 = -1;
  if (start + n <= r->capacity) {
    hi0 = lo0 + n - 1;
  } else {
    hi0 = r->tree_start + r->capacity - 1;
    lo1 = r->tree_start;
    hi1 = r->tree_start + (start + n - r->capacity) - 1;
  }
  auto up = [&]() {                              // both node ranges one level up
    lo0 = (lo0 - 1) / 2; hi0 = (hi0 - 1) / 2;
    if (hi1 >= lo1) { lo1 = (lo1 - 1) / 2; hi1 = (hi1 - 1) / 2; }
  };
  up();                                          // parents of the leaf ranges
  for (;;) {
    const int64_t cnt = (hi0 - lo0 + 1) + (hi1 >= lo1 ? hi1 - lo1 + 1 : 0);
    if (cnt <= 2048 || lo0 == 0) break;
    const int g = (int)rb_div_up(cnt, 256);
    RB_LAUNCH(k_rebuild_ranges, dim3(g > 2048 ? 2048 : g), dim3(256), stream, r->tree, lo0, hi0, lo1, hi1);
    RB_LAUNCH_CHECK();
    up();
  }
  const int64_t new_index = (start + n) % r->capacity;
  const int32_t set_full = (start + n >= r->capacity) ? 1 : 0;
  RB_LAUNCH(k_rebuild_top, dim3(1), dim3(1024), stream, v, lo0, hi0, lo1, hi1, 1, new_index, set_full);
  RB_LAUNCH_CHECK();
  r->host_index = new_index;
  if (set_full) r->host_full = 1;
  return RB_OK;
}

int rb_replay_append_streams(rb_replay_t* r, const float* states_dev, const int32_t* timesteps_host, const int32_t* actions_host,
                             const float* rewards_host, const uint8_t* nonterminals_host, rb_stream_t stream) {
  AppendRound a;
  memset(&a, 0, sizeof(a));
  const bool have = r && timesteps_host && actions_host && rewards_host && nonterminals_host;
  for (int s = 0; have && s < r->streams; ++s) {      // by value: the caller's arrays are free again when this returns
    a.timestep[s] = timesteps_host[s];
    a.action[s] = actions_host[s];
    a.reward[s] = rewards_host[s];
    a.nonterminal[s] = nonterminals_host[s] ? 1 : 0;
  }
  return append_round(r, "rb_replay_append_streams", "append:k_append_streams", states_dev, have ? &a : nullptr, stream);
}

int rb_replay_append_streams_dev(rb_replay_t* r, const float* states_dev, int32_t* timesteps_dev, const int32_t* actions_dev,
                                 const float* rewards_dev, const uint8_t* nonterminals_dev, rb_stream_t stream) {
  AppendRoundDev a;
  a.timestep = timesteps_dev; a.action = actions_dev; a.reward = rewards_dev; a.nonterminal = nonterminals_dev;
  const bool have = timesteps_dev && actions_dev && rewards_dev && nonterminals_dev;
  return append_round(r, "rb_replay_append_streams_dev", "append:k_append_streams_dev", states_dev, have ? &a : nullptr, stream);
}

// --------------------------------------------------------------- draw / update --
int rb_replay_set_beta_source(rb_replay_t* r, const float* neg_beta_dev) {
  RB_REQUIRE(r != nullptr, "rb_replay_set_beta_source: NULL handle");
  r->neg_beta_dev = neg_beta_dev;
  return RB_OK;
}

// The effective horizon and the discount of a live replay (include/rainbow_hip.h): from the next draw on the batch is the one a
// replay created with multi_step = n_eff and this discount draws from the same ring, tree and uniforms.  Allocations, the row stride
// of the window table (history + the multi_step of creation) and rb_replay_buffers_t.window_len do not change.
int rb_replay_set_horizon(rb_replay_t* r, int32_t n_eff, double discount, rb_stream_t stream) {
  RB_REQUIRE(r != nullptr, "rb_replay_set_horizon: NULL handle");
  RB_REQUIRE(n_eff >= 1 && n_eff <= r->n, "rb_replay_set_horizon: n_eff must be in [1, %d] (the multi_step the replay was created "
             "with), got %d", (int)r->n, (int)n_eff);
  RB_REQUIRE(discount > 0.0 && discount <= 1.0, "rb_replay_set_horizon: discount must be in (0, 1], got %g", discount);   // (also NaN)
  RB_SPEC_JOIN(r);                // a tentative early draw made under the old horizon is never accepted
  ++r->mutations;
  HorizonTable tab;
  memset(&tab, 0, sizeof(tab));
  for (int k = 0; k < r->n; ++k) tab.s[k] = (float)pow(discount, (double)k);  // memory.py:101, as create_impl
  tab.s[RB_STRIDE_SLOT] = r->scaling[RB_STRIDE_SLOT];                         // the row stride stays (its bits, not a float value)
  RB_LAUNCH(k_set_horizon, dim3(1), dim3(64), stream, r->scaling_dev, tab);
  RB_LAUNCH_CHECK();
  memcpy(r->scaling, tab.s, sizeof(tab.s));
  r->n_eff = n_eff; r->discount = discount;
  return RB_OK;
}

int rb_replay_get_horizon(rb_replay_t* r, int32_t* n_eff, double* discount) {
  RB_REQUIRE(r && n_eff && discount, "rb_replay_get_horizon: NULL argument");
  *n_eff = r->n_eff; *discount = r->discount;
  return RB_OK;
}

int rb_replay_find(rb_replay_t* r, const double* values_dev, int32_t n, float* probs_dev, int64_t* data_idx_dev,
                   int64_t* tree_idx_dev, rb_stream_t stream) {
  RB_REQUIRE(r && values_dev && probs_dev && data_idx_dev && tree_idx_dev, "rb_replay_find: NULL argument");
  RB_SPEC_JOIN(r);
  if (n <= 0) return RB_OK;
  RB_LAUNCH(k_find, dim3((unsigned)rb_div_up(n, 256)), dim3(256), stream, view_of(r), values_dev, n, probs_dev,
            data_idx_dev, tree_idx_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

// the frame stacks of a drawn batch, where the caller wants them (NULL: the learner reads the ring through the window table)
static int launch_gather(const ReplayView& v, int32_t win_stride, int32_t batch, const int32_t* win, uint8_t* states_dev,
                         uint8_t* next_states_dev, rb_stream_t stream) {
  if (!states_dev || !next_states_dev) return RB_OK;
  RB_LAUNCH(k_gather_stacks, dim3((unsigned)(batch * 2 * v.history)), dim3(256), stream, v, batch, win, win_stride, states_dev, next_states_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

static int sample_impl(rb_replay_t* r, int32_t batch, double priority_weight, const double* unit_uniforms_dev,
                       int32_t max_attempts, int64_t* tree_idx_dev, uint8_t* states_dev, uint8_t* next_states_dev,
                       int64_t* actions_dev, float* returns_dev, float* nonterminals_dev, float* weights_dev,
                       const rb_noise_job_t* noise_job, rb_stream_t stream) {
  RB_REQUIRE(r && tree_idx_dev && actions_dev && returns_dev && nonterminals_dev && weights_dev,
             "rb_replay_sample: NULL argument");
  RB_REQUIRE(batch >= 1 && batch <= r->max_batch, "rb_replay_sample: batch must be in [1,%d]", r->max_batch);
  RB_REQUIRE(max_attempts >= 1, "rb_replay_sample: max_attempts must be >= 1");
  RB_REQUIRE(r->capacity > (int64_t)r->history + r->n,
             "rb_replay_sample: capacity must exceed history + multi_step (no window can clear the write head otherwise: "
             "the reference's rejection loop, memory.py:128-132, would never end)");
  // an early draw in flight (rb_replay_spec_launch): this launch's sampler workgroup waits for it and either ACCEPTS it — only when
  // the caller is rb_learner_train_step (spec_accept_armed: it reads the table of THIS draw; the public entry points hand out
  // table 0, rb_replay_buffers_t.window_dev, so for them the draw is always made again, into table 0), same batch, beta, attempt
  // bound and output buffers, device RNG, nothing else has touched the replay since (every other entry point cancels it) — or draws
  // again; either way the stream-2 work is complete before anything of this stream goes on.
  const int accept_armed = r->spec_accept_armed;
  r->spec_accept_armed = 0;
  int spec_mode = 0;
  int win_set = 0;
  if (r->spec_inflight) {
    // (a captured launch never accepts: mode 3 bakes "wait for the record of epoch E, then draw" into the graph, and on every
    // replay that record is long complete)
    const bool same = accept_armed && !rb_stream_capturing(stream) && unit_uniforms_dev == nullptr && r->spec_args.batch == batch && r->spec_args.beta == priority_weight &&
                      r->spec_args.max_attempts == max_attempts && r->spec_args.tree_idx == tree_idx_dev &&
                      r->spec_args.actions == actions_dev && r->spec_args.returns == returns_dev &&
                      r->spec_args.nonterm == nonterminals_dev && r->spec_args.weights == weights_dev;
    spec_mode = same ? 2 : 3;
    if (same) win_set = r->spec_args.win_set;
    r->spec_inflight = 0;
  }
  r->win_sel = win_set;
  ++r->mutations;
  int32_t* const win_cur = win_of(r, win_set);
  const ReplayView v = view_of(r);
  // weights ** -beta: python float exponent is cast to float32 by numpy (NEP 50 weak scalar)
  const float neg_beta = (float)(-priority_weight);
  NoiseJob job;
  memset(&job, 0, sizeof(job));
  unsigned blocks = 1;
  if (noise_job) {
    memcpy(&job, noise_job, sizeof(job));
    RB_REQUIRE(job.noise && job.ctr && job.nblk > 0 && job.nets >= 1 && job.dev, "rb_replay_sample_fused_noise: empty noise job");
    blocks += (unsigned)(job.nblk * job.nets);
  }
  const int noise_blocks = (int)blocks - 1;
  // ---- the launch decision
  int threads = (int)(rb_div_up(batch, 64) * 64);
  if (threads < 256) threads = 256;   // enough lanes to stage the 16 KB tree top into LDS in one sweep
  const int window = r->history + r->n;
  const ClipAdamArgs* adam_dev = nullptr;
  if (noise_job && job.adam_dev && job.adam_blocks > 0) {      // a pending optimiser pass comes with the job
    RB_REQUIRE(threads == 256, "rb_replay_sample_fused_noise: the hosted optimiser pass needs a 256-thread sampler launch (batch <= 256)");
    adam_dev = static_cast<const ClipAdamArgs*>(job.adam_dev);
  }
  // the host is the 1024-thread sampler variant (four tree levels per trip, 127 VGPRs -> 4 waves per SIMD for the hosted
  // streaming workgroups; under the 256-thread variant's 205 VGPRs the pass took 46 us instead of 38) with 4 quadruples per
  // hosted thread — job.adam_blocks counts blocks of 4 quadruples per thread.  That variant holds windows of up to 24
  // transitions; a longer window (history + multi_step > 24) gets the pending pass as a launch of its own in front of an
  // un-hosted sampler: same order in the stream, same results.
  const bool hosted = adam_dev && window <= 24;
  const bool wide = threads > 256 || hosted;                   // k_sample<1024, RB_HOST_AU_WIDE>, otherwise k_sample<256, 8>
  RB_REQUIRE(!wide || window <= 24, "rb_replay_sample: the 1024-thread sampler (batch > 256) supports history + multi_step <= 24");
  if (hosted) {
    blocks += (unsigned)((job.adam_blocks * 4 + RB_HOST_AU_WIDE - 1) / RB_HOST_AU_WIDE);
  } else if (adam_dev) {
    const int rc = rb_launch_adam_pending(adam_dev, job.adam_blocks, stream, job.adam_ema != 0);
    if (rc != RB_OK) return rc;
    adam_dev = nullptr;
  }
  // (the tree search keeps its top 4095 nodes in LDS: measured against an all-global search, B = 32 / 1M leaves: 11.1 vs
  // 11.6 us, n = 20 / 100k: 14.3 vs 16.1, B = 256: 20.0 vs 24.4 — a trip costs ~1.3 us of issue, more than the staging)
  // (always 1, and it stays an argument, rb_tree_descend_global with it: without it k_sample<256, 8> compiled — cross-compiled, not run —
  // to a 68-byte scratch segment, which no kernel of the step may have: DESIGN.md §6)
  const int lds_top = 1;
  auto launch = [&](auto kernel) {
    RB_LAUNCH_T("sample:k_sample", kernel, dim3(blocks), dim3(threads), stream, v, batch, neg_beta, r->neg_beta_dev, unit_uniforms_dev,
                max_attempts, r->seed, r->scaling_dev, tree_idx_dev, win_cur, actions_dev, returns_dev, nonterminals_dev, weights_dev,
                job.dev, job.noise, job.noise2, job.ctr, r->fail_host, lds_top, noise_blocks, adam_dev, r->spec_res, r->spec_epoch,
                spec_mode);
  };
  if (hosted && job.adam_ema) launch(k_sample<1024, RB_HOST_AU_WIDE, true>);    // the pass moves the target network as well
  else if (wide) launch(k_sample<1024, RB_HOST_AU_WIDE>);
  else launch(k_sample<256, 8>);
  RB_LAUNCH_CHECK();
  return launch_gather(v, r->history + r->n, batch, win_cur, states_dev, next_states_dev, stream);
}

int rb_replay_sample(rb_replay_t* r, int32_t batch, double priority_weight, const double* unit_uniforms_dev,
                     int32_t max_attempts, int64_t* tree_idx_dev, uint8_t* states_dev, uint8_t* next_states_dev,
                     int64_t* actions_dev, float* returns_dev, float* nonterminals_dev, float* weights_dev,
                     rb_stream_t stream) {
  return sample_impl(r, batch, priority_weight, unit_uniforms_dev, max_attempts, tree_idx_dev, states_dev, next_states_dev,
                     actions_dev, returns_dev, nonterminals_dev, weights_dev, nullptr, stream);
}

int rb_replay_sample_fused_noise(rb_replay_t* r, int32_t batch, double priority_weight, const double* unit_uniforms_dev,
                                 int32_t max_attempts, int64_t* tree_idx_dev, uint8_t* states_dev, uint8_t* next_states_dev,
                                 int64_t* actions_dev, float* returns_dev, float* nonterminals_dev, float* weights_dev,
                                 const rb_noise_job_t* noise_job, rb_stream_t stream) {
  RB_REQUIRE(noise_job != nullptr, "rb_replay_sample_fused_noise: noise_job is NULL");
  return sample_impl(r, batch, priority_weight, unit_uniforms_dev, max_attempts, tree_idx_dev, states_dev, next_states_dev,
                     actions_dev, returns_dev, nonterminals_dev, weights_dev, noise_job, stream);
}

static int rb_update_impl(rb_replay_t* r, const int64_t* tree_idx_dev, const float* values_dev, int32_t n,
                          int32_t apply_pow, rb_stream_t stream) {
  RB_REQUIRE(r && tree_idx_dev && values_dev, "rb_replay_update: NULL argument");
  RB_REQUIRE(n >= 1 && n <= 1024, "rb_replay_update: n must be in [1,1024]");
  RB_SPEC_JOIN(r);
  ++r->mutations;
  int threads = (int)(rb_div_up(n, 64) * 64);
  if (threads < 256) threads = 256;     // the dense rebuild of the tree top wants lanes, not just one per leaf
  RB_LAUNCH(k_update, dim3(1), dim3(threads), stream, view_of(r), tree_idx_dev, values_dev, n, apply_pow, r->omega);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

int rb_replay_update_leaves(rb_replay_t* r, const int64_t* tree_idx_dev, const float* values_dev, int32_t n,
                            rb_stream_t stream) {
  return rb_update_impl(r, tree_idx_dev, values_dev, n, 0, stream);
}

int rb_replay_update_priorities(rb_replay_t* r, const int64_t* tree_idx_dev, const float* losses_dev, int32_t n,
                                rb_stream_t stream) {
  return rb_update_impl(r, tree_idx_dev, losses_dev, n, 1, stream);
}

int rb_replay_update_sample(rb_replay_t* r, const int64_t* upd_tree_idx_dev, const float* upd_losses_dev, int32_t upd_n,
                            int32_t batch, double priority_weight, const double* unit_uniforms_dev, int32_t max_attempts,
                            int64_t* tree_idx_dev, uint8_t* states_dev, uint8_t* next_states_dev, int64_t* actions_dev,
                            float* returns_dev, float* nonterminals_dev, float* weights_dev, rb_stream_t stream) {
  RB_REQUIRE(r && upd_tree_idx_dev && upd_losses_dev, "rb_replay_update_sample: NULL argument");
  RB_REQUIRE(upd_n >= 1 && upd_n <= 1024, "rb_replay_update_sample: upd_n must be in [1,1024]");
  // one launch for what a PER loop at the reference's batch sizes produces (a sorted write-back of at most 64 leaves rides on
  // one wave); longer write-backs want the 1024-thread hashed kernel (batch 256: 34 us as two launches, 50 us fused)
  if (upd_n > 64 || batch > 256) {
    const int rc = rb_update_impl(r, upd_tree_idx_dev, upd_losses_dev, upd_n, 1, stream);
    if (rc != RB_OK) return rc;
    return sample_impl(r, batch, priority_weight, unit_uniforms_dev, max_attempts, tree_idx_dev, states_dev, next_states_dev,
                       actions_dev, returns_dev, nonterminals_dev, weights_dev, nullptr, stream);
  }
  RB_REQUIRE(tree_idx_dev && actions_dev && returns_dev && nonterminals_dev && weights_dev, "rb_replay_update_sample: NULL argument");
  RB_REQUIRE(batch >= 1, "rb_replay_update_sample: batch must be in [1,%d]", r->max_batch);
  RB_REQUIRE(max_attempts >= 1, "rb_replay_update_sample: max_attempts must be >= 1");
  RB_REQUIRE(r->capacity > (int64_t)r->history + r->n, "rb_replay_update_sample: capacity must exceed history + multi_step");
  RB_SPEC_JOIN(r);
  ++r->mutations;
  r->win_sel = 0;
  const ReplayView v = view_of(r);
  const float neg_beta = (float)(-priority_weight);
  RB_LAUNCH_T("sample:k_update_sample", k_update_sample, dim3(1), dim3(256), stream, v, upd_tree_idx_dev, upd_losses_dev, upd_n, 1, r->omega,
              batch, neg_beta, r->neg_beta_dev, unit_uniforms_dev, max_attempts, r->seed, r->scaling_dev, tree_idx_dev, r->win, actions_dev,
              returns_dev, nonterminals_dev, weights_dev, r->fail_host, (SpecResult*)nullptr, 0u);
  RB_LAUNCH_CHECK();
  return launch_gather(v, r->history + r->n, batch, r->win, states_dev, next_states_dev, stream);
}

// The frame stacks of the LAST draw on the handle with random-shift augmentation (replay_shift.h): reads the window table that draw
// wrote, the ring and nothing else — no mutation of the replay, the header (rng_counter included) untouched.  After a draw that gave
// up the table holds that draw's windows and they are gathered, as rb_replay_sample's own gather does.
int rb_replay_gather_shifted(rb_replay_t* r, int32_t batch, int32_t pad, uint64_t draw, const int8_t* shifts_in_dev,
                             uint8_t* states_dev, uint8_t* next_states_dev, int8_t* shifts_out_dev, rb_stream_t stream) {
  RB_REQUIRE(r != nullptr, "rb_replay_gather_shifted: NULL handle");
  RB_REQUIRE(states_dev != nullptr, "rb_replay_gather_shifted: states_dev is NULL");
  RB_REQUIRE(next_states_dev != nullptr, "rb_replay_gather_shifted: next_states_dev is NULL");
  RB_REQUIRE(batch >= 1 && batch <= r->max_batch, "rb_replay_gather_shifted: batch must be in [1,%d], got %d", r->max_batch, (int)batch);
  RB_REQUIRE(pad >= 0 && pad <= RB_SHIFT_MAX_PAD, "rb_replay_gather_shifted: pad must be in [0,%d], got %d", RB_SHIFT_MAX_PAD, (int)pad);
  RB_REQUIRE((((uintptr_t)states_dev | (uintptr_t)next_states_dev) & 15u) == 0,
             "rb_replay_gather_shifted: states_dev and next_states_dev must be 16-byte aligned");
  RB_SPEC_JOIN(r);
  RB_LAUNCH_T("sample:k_gather_stacks_shift", k_gather_stacks_shift, dim3((unsigned)(batch * 2 * r->history)), dim3(256), stream, view_of(r),
              batch, win_of(r, r->win_sel), r->history + r->n, pad, r->seed ^ RB_SHIFT_KEY_TAG, draw, shifts_in_dev, states_dev, next_states_dev,
              shifts_out_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

// ------------------------------------------------------------- validation view --
int rb_replay_state_at(rb_replay_t* r, int64_t data_index, float* out_dev, rb_stream_t stream) {
  RB_REQUIRE(r && out_dev, "rb_replay_state_at: NULL argument");
  RB_SPEC_JOIN(r);
  RB_REQUIRE(data_index >= 0 && data_index < r->capacity, "rb_replay_state_at: index out of range");
  RB_LAUNCH(k_state_at, dim3(1), dim3(256), stream, view_of(r), data_index, out_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

int rb_replay_states_at(rb_replay_t* r, const int64_t* data_index_dev, int32_t n, float* out_dev, rb_stream_t stream) {
  RB_REQUIRE(r && data_index_dev && out_dev, "rb_replay_states_at: NULL argument");
  RB_SPEC_JOIN(r);
  RB_REQUIRE(n >= 0, "rb_replay_states_at: n must be >= 0");
  if (n == 0) return RB_OK;
  RB_LAUNCH(k_states_at, dim3((unsigned)n), dim3(256), stream, view_of(r), data_index_dev, out_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

// ---------------------------------------------------------------------- counters --
// The shape of the priority distribution (include/rainbow_hip.h; replay_stats.h k_priority_stats): a read of the leaves, in stream order.
int rb_replay_priority_stats(rb_replay_t* r, rb_priority_stats_t* out_dev, rb_stream_t stream) {
  RB_REQUIRE(r != nullptr, "rb_replay_priority_stats: NULL handle (r)");
  RB_REQUIRE(out_dev != nullptr, "rb_replay_priority_stats: NULL out_dev");
  RB_SPEC_JOIN(r);
  if (!r->pstats) {
    RB_HIP_TRY(rb_dev_malloc((void**)&r->pstats, sizeof(PriorityScratch)));
    RB_HIP_TRY(hipMemset(r->pstats, 0, sizeof(PriorityScratch)));      // the counters start at zero and put themselves back
  }
  PriorityStatsArgs a;
  a.leaves = r->tree + r->tree_start; a.capacity = r->capacity;
  a.chunk = rb_div_up(rb_div_up(r->capacity, RB_PSTATS_MAX_WG), RB_PSTATS_THREADS) * RB_PSTATS_THREADS;
  if (a.chunk < RB_PSTATS_MIN_CHUNK) a.chunk = RB_PSTATS_MIN_CHUNK;
  a.scratch = r->pstats; a.out = out_dev;
  RB_LAUNCH(k_priority_stats, dim3((unsigned)rb_div_up(r->capacity, a.chunk)), dim3(RB_PSTATS_THREADS), stream, a);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

int rb_replay_streams(rb_replay_t* r, int32_t* streams) {
  RB_REQUIRE(r && streams, "rb_replay_streams: NULL argument");
  *streams = r->streams;
  return RB_OK;
}

#if defined(RB_STAMP)
int rb_debug_stamps(long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamp), sizeof(long long) * 32) == hipSuccess ? 0 : -2; }
#endif
// word `which` of the pinned host block the kernels count in (rb_replay.fail_host): no synchronisation
static int read_counter(rb_replay_t* r, int64_t* count, int which, const char* entry) {
  RB_REQUIRE(r && count, "%s: NULL argument", entry);
  *count = (int64_t)*(volatile int32_t*)(r->fail_host + which);
  return RB_OK;
}
int rb_replay_failed_samples(rb_replay_t* r, int64_t* count) { return read_counter(r, count, 0, "rb_replay_failed_samples"); }
int rb_replay_dropped_updates(rb_replay_t* r, int64_t* count) { return read_counter(r, count, 1, "rb_replay_dropped_updates"); }
int rb_replay_expired_waits(rb_replay_t* r, int64_t* count) { return read_counter(r, count, 2, "rb_replay_expired_waits"); }

int rb_replay_reset_failed_samples(rb_replay_t* r) {
  RB_REQUIRE(r != nullptr, "rb_replay_reset_failed_samples: NULL handle");
  RB_SPEC_JOIN(r);                             // (an early pair in flight may still count)
  *(volatile int32_t*)r->fail_host = 0;        // (a failed launch still in flight re-increments it when it completes)
  *(volatile int32_t*)(r->fail_host + 1) = 0;
  *(volatile int32_t*)(r->fail_host + 2) = 0;
  r->spec_disabled = 0;
  return RB_OK;
}

int rb_replay_position(rb_replay_t* r, int64_t* index, int32_t* full) {
  RB_REQUIRE(r != nullptr, "rb_replay_position: NULL handle");
  if (index) *index = r->host_index;
  if (full) *full = r->host_full;
  return RB_OK;
}

}  // extern "C"
