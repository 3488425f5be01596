// episode_tally.h — per-episode returns of S environment streams, recorded on the device (rb_tally_*; the rules are in
// include/rainbow_hip.h).  Part of vec_env.hip, included there and nowhere else.
//
// The recorder is fed with the rewards / nonterminals vectors a round already produces (rb_catch_step, or any other device
// environment), so an evaluation round stays launches on one stream: act -> step -> tally.  One wave, one lane per stream:
// 12 bytes of running state per stream, at most one (return, length) record written per stream and step.
#pragma once
#include "rb_common.h"

#include <new>

#define RB_TALLY_MAX_EPISODES 65536

struct TallyStream {
  float ret;          // return of the episode in play
  int32_t len;        // its steps so far
  int32_t recorded;   // episodes of this stream on record (<= its quota)
  int32_t pad_;
};

struct rb_tally {
  int32_t streams, episodes;
  void* block;             // one device allocation: the four arrays below
  TallyStream* state;      // [S]
  float* returns;          // [episodes], stream-major: stream s owns [offset(s), offset(s) + quota(s))
  int32_t* lengths;        // [episodes]
  int32_t* remaining;      // [1]
};

// quota(s) = E / S + (s < E % S); offset(s) = sum of the quotas before s
__host__ __device__ __forceinline__ int rb_tally_quota(int S, int E, int s) { return E / S + (s < E % S ? 1 : 0); }
__host__ __device__ __forceinline__ int rb_tally_offset(int S, int E, int s) { return s * (E / S) + (s < E % S ? s : E % S); }

__global__ __launch_bounds__(256) void k_tally_reset(TallyStream* state, float* returns, int32_t* lengths, int32_t* remaining, int S,
                                                      int E) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < S) { state[i].ret = 0.0f; state[i].len = 0; state[i].recorded = 0; state[i].pad_ = 0; }
  if (i < E) { returns[i] = __builtin_nanf(""); lengths[i] = 0; }
  if (i == 0) *remaining = E;
}

// grid = 1, block = 64: lane s is stream s
__global__ __launch_bounds__(64) void k_tally_step(TallyStream* state, float* returns, int32_t* lengths, int32_t* remaining, int S,
                                                    int E, const float* rewards, const uint8_t* nonterminals) {
  const int s = rb_lane();
  float need = 0.0f;
  if (s < S) {
    const TallyStream cur = state[s];
    const int quota = rb_tally_quota(S, E, s);
    float ret = cur.ret + rewards[s];                        // the ending step's reward belongs to the ending episode
    int len = cur.len + 1, rec = cur.recorded;
    if (nonterminals[s] == 0) {
      if (rec < quota) {                                     // rec < quota: the slot lies inside this stream's range, below E
        const int slot = rb_tally_offset(S, E, s) + rec;
        returns[slot] = ret;
        lengths[slot] = len;
        ++rec;
      }
      ret = 0.0f;
      len = 0;
    }
    TallyStream nx;
    nx.ret = ret; nx.len = len; nx.recorded = rec; nx.pad_ = 0;
    state[s] = nx;
    need = (float)(quota - rec);
  }
  const float total = rb_wave_sum(need);                     // <= 65536: exact in f32
  if (s == 0) *remaining = (int32_t)total;
}

extern "C" {

int rb_tally_create(rb_tally_t** out, int32_t streams, int32_t episodes) {
  RB_REQUIRE(out, "rb_tally_create: NULL argument");
  *out = nullptr;
  RB_REQUIRE(streams >= 1 && streams <= RB_MAX_STREAMS, "rb_tally_create: streams must be in [1, %d], got %d", RB_MAX_STREAMS,
             (int)streams);
  RB_REQUIRE(episodes >= 1 && episodes <= RB_TALLY_MAX_EPISODES, "rb_tally_create: episodes must be in [1, %d], got %d",
             RB_TALLY_MAX_EPISODES, (int)episodes);
  rb_tally* t = new (std::nothrow) rb_tally();
  if (!t) { rb_set_error("rb_tally_create: out of host memory"); return RB_ERR_OOM; }
  t->streams = streams; t->episodes = episodes; t->block = nullptr;
  const size_t state_bytes = sizeof(TallyStream) * (size_t)streams, rec_bytes = 4 * (size_t)episodes;
  if (rb_dev_malloc(&t->block, state_bytes + 2 * rec_bytes + 16) != hipSuccess) {
    delete t;
    rb_set_error("rb_tally_create: device allocation failed");
    return RB_ERR_OOM;
  }
  char* p = (char*)t->block;
  t->state = (TallyStream*)p;
  t->returns = (float*)(p + state_bytes);
  t->lengths = (int32_t*)(p + state_bytes + rec_bytes);
  t->remaining = (int32_t*)(p + state_bytes + 2 * rec_bytes);
  int rc = rb_tally_reset(t, nullptr);
  if (rc == RB_OK && hipStreamSynchronize((hipStream_t) nullptr) != hipSuccess) {
    rb_set_error("rb_tally_create: the first reset failed");
    rc = RB_ERR_HIP;
  }
  if (rc != RB_OK) {
    rb_dev_free(t->block);
    delete t;
    return rc;
  }
  *out = t;
  return RB_OK;
}

int rb_tally_destroy(rb_tally_t* t) {
  if (!t) return RB_OK;
  if (t->block) rb_dev_free(t->block);
  delete t;
  return RB_OK;
}

int rb_tally_reset(rb_tally_t* t, rb_stream_t stream) {
  RB_REQUIRE(t, "rb_tally_reset: NULL argument");
  const int n = t->episodes > t->streams ? t->episodes : t->streams;
  RB_LAUNCH(k_tally_reset, dim3((unsigned)rb_div_up(n, 256)), dim3(256), stream, t->state, t->returns, t->lengths, t->remaining,
            (int)t->streams, (int)t->episodes);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

int rb_tally_step(rb_tally_t* t, const float* rewards_dev, const uint8_t* nonterminals_dev, rb_stream_t stream) {
  RB_REQUIRE(t && rewards_dev && nonterminals_dev, "rb_tally_step: NULL argument");
  RB_LAUNCH(k_tally_step, dim3(1), dim3(64), stream, t->state, t->returns, t->lengths, t->remaining, (int)t->streams, (int)t->episodes,
            rewards_dev, nonterminals_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

int rb_tally_remaining(rb_tally_t* t, int32_t* remaining_host, rb_stream_t stream) {
  RB_REQUIRE(t && remaining_host, "rb_tally_remaining: NULL argument");
  RB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  RB_HIP_TRY(hipMemcpy(remaining_host, t->remaining, sizeof(int32_t), hipMemcpyDeviceToHost));
  return RB_OK;
}

int rb_tally_read(rb_tally_t* t, float* returns_host, int32_t* lengths_host, int32_t* streams_host, rb_stream_t stream) {
  RB_REQUIRE(t && returns_host && lengths_host && streams_host, "rb_tally_read: NULL argument");
  RB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  RB_HIP_TRY(hipMemcpy(returns_host, t->returns, 4 * (size_t)t->episodes, hipMemcpyDeviceToHost));
  RB_HIP_TRY(hipMemcpy(lengths_host, t->lengths, 4 * (size_t)t->episodes, hipMemcpyDeviceToHost));
  for (int s = 0; s < t->streams; ++s) {
    const int off = rb_tally_offset(t->streams, t->episodes, s), q = rb_tally_quota(t->streams, t->episodes, s);
    for (int k = 0; k < q; ++k) streams_host[off + k] = s;
  }
  return RB_OK;
}

}  // extern "C"
