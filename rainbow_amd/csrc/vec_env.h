// vec_env.h — environments that live on the device (the whole of vec_env.hip; the rules of the game are in include/rainbow_hip.h).
//
// Catch on the 84 x 84 screen, S independent streams, one 256-thread workgroup per stream.  A step is a tiny, latency-bound
// launch: 16 bytes of game state per stream, then history frames of 28 KB written with 16-byte lanes (the shifted stack is
// a straight copy, the new observation is rendered from three integers).  Nothing is read back by the host: rewards,
// nonterminals and the next stacks go to device arrays, the episode totals accumulate per stream in the state block.
#pragma once
#include "rb_common.h"

#include <string.h>

#define RB_CATCH_GRID 12
#define RB_CATCH_CELL 7
#define RB_CATCH_PADDLE 3
#define RB_CATCH_MAX_HISTORY 16

struct CatchStream {
  int32_t ball_col, ball_row, paddle;   // paddle = its left cell, in [0, GRID - PADDLE]
  uint32_t episode;                     // number of the episode in play (0xFFFFFFFF before the first reset)
  int32_t episodes_done, catches, return_sum, pad_;
};

struct rb_catch {
  int32_t streams, history;
  uint64_t seed;
  CatchStream* state;   // device [S]
  int reset_done;
};

// start of episode `e` of stream `s`: ball column and paddle position from one Philox block
__device__ __forceinline__ void rb_catch_begin(uint64_t seed, int s, uint32_t e, int* ball_col, int* paddle) {
  const rb_philox_out r = rb_philox(seed, (uint64_t)s, (uint64_t)e);
  *ball_col = (int)(r.v[0] % (uint32_t)RB_CATCH_GRID);
  *paddle = (int)(r.v[1] % (uint32_t)(RB_CATCH_GRID - RB_CATCH_PADDLE + 1));
}

__device__ __forceinline__ float rb_catch_pixel(int p, int ball_col, int ball_row, int paddle) {
  const int y = p / RB_FRAME_W, x = p - y * RB_FRAME_W;
  const int cr = y / RB_CATCH_CELL, cc = x / RB_CATCH_CELL;
  if (cr == ball_row && cc == ball_col) return 1.0f;
  if (cr == RB_CATCH_GRID - 1 && cc >= paddle && cc < paddle + RB_CATCH_PADDLE) return 0.5f;
  return 0.0f;
}
// one frame (7056 floats, 16-byte lanes) by the whole workgroup
__device__ __forceinline__ void rb_catch_render(float* frame, int ball_col, int ball_row, int paddle) {
  float4* dst = (float4*)frame;
  for (int w = (int)threadIdx.x; w < RB_FRAME_BYTES / 4; w += (int)blockDim.x) {
    const int p = 4 * w;
    dst[w] = make_float4(rb_catch_pixel(p, ball_col, ball_row, paddle), rb_catch_pixel(p + 1, ball_col, ball_row, paddle),
                         rb_catch_pixel(p + 2, ball_col, ball_row, paddle), rb_catch_pixel(p + 3, ball_col, ball_row, paddle));
  }
}
// the reset stack (env.py:44-52): history - 1 blank frames, then the first observation
__device__ __forceinline__ void rb_catch_reset_stack(float* stack, int history, int ball_col, int paddle) {
  float4* dst = (float4*)stack;
  const int blank = (history - 1) * (RB_FRAME_BYTES / 4);
  for (int w = (int)threadIdx.x; w < blank; w += (int)blockDim.x) dst[w] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  rb_catch_render(stack + (int64_t)(history - 1) * RB_FRAME_BYTES, ball_col, 0, paddle);
}

__global__ __launch_bounds__(256) void k_catch_reset(CatchStream* state, uint64_t seed, int history, float* stacks) {
  const int s = (int)blockIdx.x;
  const uint32_t e = state[s].episode + 1u;
  __syncthreads();                      // every thread has read the episode number before thread 0 rewrites it
  int ball_col, paddle;
  rb_catch_begin(seed, s, e, &ball_col, &paddle);
  if (threadIdx.x == 0) {
    state[s].ball_col = ball_col; state[s].ball_row = 0; state[s].paddle = paddle; state[s].episode = e;
  }
  rb_catch_reset_stack(stacks + (int64_t)s * history * RB_FRAME_BYTES, history, ball_col, paddle);
}

__global__ __launch_bounds__(256) void k_catch_step(CatchStream* state, uint64_t seed, int history, const int32_t* actions,
                                                     const float* stacks_in, float* stacks_out, float* rewards,
                                                     uint8_t* nonterminals) {
  const int s = (int)blockIdx.x;
  const CatchStream cur = state[s];
  __syncthreads();                      // every thread holds the old state before thread 0 rewrites it
  const int32_t a = actions[s];
  int paddle = cur.paddle;
  if (a == 1) paddle = paddle > 0 ? paddle - 1 : 0;
  else if (a == 2) paddle = paddle < RB_CATCH_GRID - RB_CATCH_PADDLE ? paddle + 1 : RB_CATCH_GRID - RB_CATCH_PADDLE;
  const int ball_row = cur.ball_row + 1;
  const bool done = ball_row >= RB_CATCH_GRID - 1;
  float* out = stacks_out + (int64_t)s * history * RB_FRAME_BYTES;
  if (!done) {
    if (threadIdx.x == 0) {
      state[s].paddle = paddle; state[s].ball_row = ball_row;
      rewards[s] = 0.0f; nonterminals[s] = 1;
    }
    const float4* src = (const float4*)(stacks_in + ((int64_t)s * history + 1) * RB_FRAME_BYTES);    // env.py:70: drop the oldest
    float4* dst = (float4*)out;
    const int moved = (history - 1) * (RB_FRAME_BYTES / 4);
    for (int w = (int)threadIdx.x; w < moved; w += (int)blockDim.x) dst[w] = src[w];
    rb_catch_render(out + (int64_t)(history - 1) * RB_FRAME_BYTES, cur.ball_col, ball_row, paddle);
    return;
  }
  const bool caught = cur.ball_col >= paddle && cur.ball_col < paddle + RB_CATCH_PADDLE;
  const uint32_t e = cur.episode + 1u;
  int ball_col, next_paddle;
  rb_catch_begin(seed, s, e, &ball_col, &next_paddle);
  if (threadIdx.x == 0) {
    CatchStream nx = cur;
    nx.ball_col = ball_col; nx.ball_row = 0; nx.paddle = next_paddle; nx.episode = e;
    nx.episodes_done = cur.episodes_done + 1;
    nx.catches = cur.catches + (caught ? 1 : 0);
    nx.return_sum = cur.return_sum + (caught ? 1 : -1);
    state[s] = nx;
    rewards[s] = caught ? 1.0f : -1.0f; nonterminals[s] = 0;
  }
  rb_catch_reset_stack(out, history, ball_col, next_paddle);
}

__global__ void k_catch_reset_stats(CatchStream* state, int S) {
  const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s < S) { state[s].episodes_done = 0; state[s].catches = 0; state[s].return_sum = 0; }
}

extern "C" {

int rb_catch_create(rb_catch_t** out, int32_t streams, int32_t history, uint64_t seed) {
  RB_REQUIRE(out, "rb_catch_create: NULL argument");
  *out = nullptr;
  RB_REQUIRE(streams >= 1 && streams <= RB_MAX_STREAMS, "rb_catch_create: streams must be in [1, %d], got %d", RB_MAX_STREAMS,
             (int)streams);
  RB_REQUIRE(history >= 1 && history <= RB_CATCH_MAX_HISTORY, "rb_catch_create: history must be in [1, %d], got %d",
             RB_CATCH_MAX_HISTORY, (int)history);
  rb_catch* c = new (std::nothrow) rb_catch();
  if (!c) { rb_set_error("rb_catch_create: out of host memory"); return RB_ERR_OOM; }
  c->streams = streams; c->history = history; c->seed = seed; c->state = nullptr; c->reset_done = 0;
  if (rb_dev_malloc((void**)&c->state, sizeof(CatchStream) * (size_t)streams) != hipSuccess) {
    delete c;
    rb_set_error("rb_catch_create: device allocation failed");
    return RB_ERR_OOM;
  }
  CatchStream init[RB_MAX_STREAMS];
  memset(init, 0, sizeof(init));
  for (int s = 0; s < streams; ++s) init[s].episode = 0xFFFFFFFFu;
  const hipError_t e = hipMemcpy(c->state, init, sizeof(CatchStream) * (size_t)streams, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    rb_dev_free(c->state);
    delete c;
    rb_set_error("rb_catch_create: hipMemcpy failed: %s", hipGetErrorString(e));
    return RB_ERR_HIP;
  }
  *out = c;
  return RB_OK;
}

int rb_catch_destroy(rb_catch_t* c) {
  if (!c) return RB_OK;
  if (c->state) rb_dev_free(c->state);
  delete c;
  return RB_OK;
}

int rb_catch_reset(rb_catch_t* c, float* stacks_dev, rb_stream_t stream) {
  RB_REQUIRE(c && stacks_dev, "rb_catch_reset: NULL argument");
  RB_REQUIRE(((uintptr_t)stacks_dev & 15u) == 0, "rb_catch_reset: stacks_dev must be 16-byte aligned");
  RB_LAUNCH(k_catch_reset, dim3((unsigned)c->streams), dim3(256), stream, c->state, c->seed, (int)c->history, stacks_dev);
  RB_LAUNCH_CHECK();
  c->reset_done = 1;
  return RB_OK;
}

int rb_catch_step(rb_catch_t* c, const int32_t* actions_dev, const float* stacks_in_dev, float* stacks_out_dev, float* rewards_dev,
                  uint8_t* nonterminals_dev, rb_stream_t stream) {
  RB_REQUIRE(c && actions_dev && stacks_in_dev && stacks_out_dev && rewards_dev && nonterminals_dev, "rb_catch_step: NULL argument");
  RB_REQUIRE((((uintptr_t)stacks_in_dev | (uintptr_t)stacks_out_dev) & 15u) == 0, "rb_catch_step: the stacks must be 16-byte aligned");
  const size_t bytes = (size_t)c->streams * (size_t)c->history * RB_FRAME_BYTES * sizeof(float);
  const uintptr_t in = (uintptr_t)stacks_in_dev, outp = (uintptr_t)stacks_out_dev;
  RB_REQUIRE(in + bytes <= outp || outp + bytes <= in, "rb_catch_step: stacks_out_dev overlaps stacks_in_dev (the step is out of place)");
  if (!c->reset_done) {
    rb_set_error("rb_catch_step: no episode in play: call rb_catch_reset first");
    return RB_ERR_STATE;
  }
  RB_LAUNCH(k_catch_step, dim3((unsigned)c->streams), dim3(256), stream, c->state, c->seed, (int)c->history, actions_dev,
            stacks_in_dev, stacks_out_dev, rewards_dev, nonterminals_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

int rb_catch_stats(rb_catch_t* c, rb_catch_stats_t* out_host, rb_stream_t stream) {
  RB_REQUIRE(c && out_host, "rb_catch_stats: NULL argument");
  CatchStream host[RB_MAX_STREAMS];
  RB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  RB_HIP_TRY(hipMemcpy(host, c->state, sizeof(CatchStream) * (size_t)c->streams, hipMemcpyDeviceToHost));
  out_host->episodes = 0; out_host->catches = 0; out_host->return_sum = 0.0;
  for (int s = 0; s < c->streams; ++s) {
    out_host->episodes += host[s].episodes_done;
    out_host->catches += host[s].catches;
    out_host->return_sum += (double)host[s].return_sum;
  }
  return RB_OK;
}

int rb_catch_reset_stats(rb_catch_t* c, rb_stream_t stream) {
  RB_REQUIRE(c, "rb_catch_reset_stats: NULL argument");
  RB_LAUNCH(k_catch_reset_stats, dim3(1), dim3(64), stream, c->state, (int)c->streams);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

}  // extern "C"
