// breakout_env.h — device Breakout with lives (a section of vec_env.hip; the rules of the game are in include/rainbow_hip.h).
//
// The pattern of vec_env.h: S independent streams, one 256-thread workgroup per stream, 64 bytes of game state per stream that
// every thread reads; the next state is computed uniformly by all threads and stored by thread 0 after a barrier.  The stack
// is moved and the new frame written with 16-byte lanes.  The frame is rendered from a table of the 144 cell intensities that
// the workgroup builds once in LDS from the NEW state (36 brick bits, paddle, ball), not from per-pixel brick tests.
#pragma once
#include "rb_common.h"

#include <string.h>

#define RB_BRK_GRID 12
#define RB_BRK_CELL 7
#define RB_BRK_PADDLE 2
#define RB_BRK_LIVES 3
#define RB_BRK_SERVE_ROW 4
#define RB_BRK_ROW_FULL 0xFFFu
#define RB_BRK_ALL_BRICKS 0xFFFFFFFFFull   // rows 1, 2, 3 as one mask: bit (r - 1) * 12 + c
#define RB_BRK_MAX_HISTORY 16
#define RB_BRK_MAX_STEPS 65535

typedef rb_breakout_state_t BreakoutStream;
static_assert(sizeof(BreakoutStream) == 64, "the state block of a stream is 64 bytes");

struct rb_breakout {
  int32_t streams, history, max_steps;
  uint64_t seed;
  BreakoutStream* state;   // device [S]
  int reset_done;
};

// (the three row masks as one 36-bit word: no indexed access to the struct's array, which would put it in scratch)
__device__ __forceinline__ uint64_t rb_brk_bricks(const BreakoutStream& st) {
  return (uint64_t)st.rows[0] | ((uint64_t)st.rows[1] << 12) | ((uint64_t)st.rows[2] << 24);
}
__device__ __forceinline__ void rb_brk_set_bricks(BreakoutStream* st, uint64_t m) {
  st->rows[0] = (uint16_t)(m & RB_BRK_ROW_FULL);
  st->rows[1] = (uint16_t)((m >> 12) & RB_BRK_ROW_FULL);
  st->rows[2] = (uint16_t)((m >> 24) & RB_BRK_ROW_FULL);
}

// the stream's next serve from one Philox block; a new game also takes its paddle from it, refills the bricks and the lives
__device__ __forceinline__ void rb_brk_serve(BreakoutStream* st, uint64_t seed, int s, bool new_game) {
  const uint32_t k = st->k + 1u;
  const rb_philox_out r = rb_philox(seed, (uint64_t)s, (uint64_t)k);
  st->k = k;
  st->bx = (int32_t)(r.v[0] % (uint32_t)RB_BRK_GRID);
  st->by = RB_BRK_SERVE_ROW;
  st->dx = (r.v[1] & 1u) ? 1 : -1;
  st->dy = 1;
  if (new_game) {
    st->paddle = (int32_t)(r.v[2] % (uint32_t)(RB_BRK_GRID - RB_BRK_PADDLE + 1));
    rb_brk_set_bricks(st, RB_BRK_ALL_BRICKS);
    st->lives = RB_BRK_LIVES;
    st->t = 0;
    st->game_return = 0;
  }
}

// the 144 cell intensities of a state, by the whole workgroup (ends with a barrier: the table is complete on return)
__device__ __forceinline__ void rb_brk_cells(float* cells, const BreakoutStream& st) {
  const uint64_t m = rb_brk_bricks(st);
  for (int i = (int)threadIdx.x; i < RB_BRK_GRID * RB_BRK_GRID; i += (int)blockDim.x) {
    const int r = i / RB_BRK_GRID, c = i - r * RB_BRK_GRID;
    const int bit = i - RB_BRK_GRID;                       // rows 1 .. 3 are bits 0 .. 35
    float v = 0.0f;
    if (bit >= 0 && bit < 3 * RB_BRK_GRID) v = ((m >> bit) & 1ull) ? 0.75f : 0.0f;
    if (r == RB_BRK_GRID - 1 && c >= st.paddle && c < st.paddle + RB_BRK_PADDLE) v = 0.5f;
    if (r == st.by && c == st.bx) v = 1.0f;
    cells[i] = v;
  }
  __syncthreads();
}
// one frame (7056 floats, 16-byte lanes) from the table: the four pixels of a lane lie in one pixel row (84 = 4 * 21)
__device__ __forceinline__ void rb_brk_render(float* frame, const float* cells) {
  float4* dst = (float4*)frame;
  constexpr int LANES_PER_ROW = RB_FRAME_W / 4;
  for (int w = (int)threadIdx.x; w < RB_FRAME_BYTES / 4; w += (int)blockDim.x) {
    const int y = w / LANES_PER_ROW, x = 4 * (w - y * LANES_PER_ROW);
    const float* row = cells + (y / RB_BRK_CELL) * RB_BRK_GRID;
    dst[w] = make_float4(row[x / RB_BRK_CELL], row[(x + 1) / RB_BRK_CELL], row[(x + 2) / RB_BRK_CELL], row[(x + 3) / RB_BRK_CELL]);
  }
}
// the reset stack (env.py:44-52): history - 1 blank frames, then the first observation
__device__ __forceinline__ void rb_brk_reset_stack(float* stack, int history, const float* cells) {
  float4* dst = (float4*)stack;
  const int blank = (history - 1) * (RB_FRAME_BYTES / 4);
  for (int w = (int)threadIdx.x; w < blank; w += (int)blockDim.x) dst[w] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  rb_brk_render(stack + (int64_t)(history - 1) * RB_FRAME_BYTES, cells);
}

__global__ __launch_bounds__(256) void k_breakout_reset(BreakoutStream* state, uint64_t seed, int history, float* stacks) {
  __shared__ float cells[RB_BRK_GRID * RB_BRK_GRID];
  const int s = (int)blockIdx.x;
  BreakoutStream st;
  st.k = state[s].k;
  __syncthreads();                      // every thread has read the serve number before thread 0 rewrites it
  rb_brk_serve(&st, seed, s, true);     // (a new game sets every field of the game; the totals stay where they are)
  if (threadIdx.x == 0) {
    BreakoutStream* d = state + s;
    d->bx = st.bx; d->by = st.by; d->dx = st.dx; d->dy = st.dy; d->paddle = st.paddle; d->t = st.t; d->k = st.k;
    d->rows[0] = st.rows[0]; d->rows[1] = st.rows[1]; d->rows[2] = st.rows[2]; d->lives = st.lives;
    d->game_return = st.game_return;
  }
  rb_brk_cells(cells, st);
  rb_brk_reset_stack(stacks + (int64_t)s * history * RB_FRAME_BYTES, history, cells);
}

__global__ __launch_bounds__(256) void k_breakout_step(BreakoutStream* state, uint64_t seed, int history, int max_steps,
                                                        int life_terminals, const int32_t* actions, const float* stacks_in,
                                                        float* stacks_out, float* rewards, uint8_t* nonterminals) {
  __shared__ float cells[RB_BRK_GRID * RB_BRK_GRID];
  const int s = (int)blockIdx.x;
  BreakoutStream st = state[s];
  __syncthreads();                      // every thread holds the old state before thread 0 rewrites it
  const int32_t a = actions[s];
  if (a == 1) st.paddle = st.paddle > 0 ? st.paddle - 1 : 0;                                                     // 1.
  else if (a == 2) st.paddle = st.paddle < RB_BRK_GRID - RB_BRK_PADDLE ? st.paddle + 1 : RB_BRK_GRID - RB_BRK_PADDLE;
  st.t += 1;                                                                                                     // 2.
  st.steps += 1;
  int reward = 0;
  bool lost = false, over = false;
  int nx = st.bx + st.dx;                                                                                        // 3.
  if (nx < 0 || nx > RB_BRK_GRID - 1) { st.dx = -st.dx; nx = st.bx + st.dx; }
  int ny = st.by + st.dy;
  if (ny < 0) { st.dy = 1; ny = st.by + st.dy; }
  uint64_t m = rb_brk_bricks(st);
  const bool brick_row = ny >= 1 && ny <= 3;
  const uint64_t brick = brick_row ? 1ull << ((ny - 1) * RB_BRK_GRID + nx) : 0ull;
  if (m & brick) {                                                                                               // 4.
    m &= ~brick;
    reward = 5 - ny;
    st.dy = -st.dy;
    st.bricks += 1;
  } else if (ny == RB_BRK_GRID - 1) {
    if (nx >= st.paddle && nx < st.paddle + RB_BRK_PADDLE) {
      st.bx = nx;
      st.dy = -1;
      st.dx = nx == st.paddle ? -1 : 1;
      if (m == 0) m = RB_BRK_ALL_BRICKS;
    } else {
      st.lives = (uint16_t)(st.lives - 1);
      st.lives_lost += 1;
      lost = true;
      over = st.lives == 0;
    }
  } else {
    st.bx = nx;
    st.by = ny;
  }
  rb_brk_set_bricks(&st, m);
  st.game_return += reward;
  if (st.t == max_steps) over = true;                                                                            // 5.
  if (over) { st.games += 1; st.return_sum += st.game_return; }
  if (over || lost) rb_brk_serve(&st, seed, s, over);                                                            // 6.
  if (threadIdx.x == 0) {
    state[s] = st;
    rewards[s] = (float)reward;
    nonterminals[s] = (over || (lost && life_terminals != 0)) ? 0 : 1;
  }
  rb_brk_cells(cells, st);
  float* out = stacks_out + (int64_t)s * history * RB_FRAME_BYTES;
  if (over) {
    rb_brk_reset_stack(out, history, cells);
  } else {
    const float4* src = (const float4*)(stacks_in + ((int64_t)s * history + 1) * RB_FRAME_BYTES);    // env.py:70: drop the oldest
    float4* dst = (float4*)out;
    const int moved = (history - 1) * (RB_FRAME_BYTES / 4);
    for (int w = (int)threadIdx.x; w < moved; w += (int)blockDim.x) dst[w] = src[w];
    rb_brk_render(out + (int64_t)(history - 1) * RB_FRAME_BYTES, cells);
  }
}

__global__ void k_breakout_reset_stats(BreakoutStream* state, int S) {
  const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s < S) { state[s].games = 0; state[s].return_sum = 0; state[s].bricks = 0; state[s].lives_lost = 0; state[s].steps = 0; }
}

// host: the first field of stream `s` that rb_breakout_set_state has to refuse (NULL = the state is a legal one)
static const char* rb_brk_invalid_field(const BreakoutStream& st, int max_steps) {
  if (st.bx < 0 || st.bx > RB_BRK_GRID - 1) return "bx must be in [0, 11]";
  if (st.by < 0 || st.by > RB_BRK_GRID - 2) return "by must be in [0, 10]";
  if (st.dx != 1 && st.dx != -1) return "dx must be -1 or +1";
  if (st.dy != 1 && st.dy != -1) return "dy must be -1 or +1";
  if (st.paddle < 0 || st.paddle > RB_BRK_GRID - RB_BRK_PADDLE) return "paddle must be in [0, 10]";
  if (st.t < 0 || st.t >= max_steps) return "t must be in [0, max_steps)";
  if (st.lives < 1 || st.lives > RB_BRK_LIVES) return "lives must be in [1, 3]";
  for (int r = 0; r < 3; ++r)
    if (st.rows[r] > RB_BRK_ROW_FULL) return "rows must be 12-bit masks";
  if (st.by >= 1 && st.by <= 3 && ((st.rows[st.by - 1] >> st.bx) & 1u)) return "the ball (bx, by) is on a brick cell";
  if (st.game_return < 0) return "game_return must be >= 0";
  if (st.games < 0 || st.return_sum < 0 || st.bricks < 0 || st.lives_lost < 0 || st.steps < 0) return "the totals must be >= 0";
  if (st.reserved != 0) return "reserved must be 0";
  return nullptr;
}

extern "C" {

int rb_breakout_create(rb_breakout_t** out, int32_t streams, int32_t history, int32_t max_steps, uint64_t seed) {
  RB_REQUIRE(out, "rb_breakout_create: NULL argument");
  *out = nullptr;
  RB_REQUIRE(streams >= 1 && streams <= RB_MAX_STREAMS, "rb_breakout_create: streams must be in [1, %d], got %d", RB_MAX_STREAMS,
             (int)streams);
  RB_REQUIRE(history >= 1 && history <= RB_BRK_MAX_HISTORY, "rb_breakout_create: history must be in [1, %d], got %d",
             RB_BRK_MAX_HISTORY, (int)history);
  RB_REQUIRE(max_steps >= 1 && max_steps <= RB_BRK_MAX_STEPS, "rb_breakout_create: max_steps must be in [1, %d], got %d",
             RB_BRK_MAX_STEPS, (int)max_steps);
  rb_breakout* c = new (std::nothrow) rb_breakout();
  if (!c) { rb_set_error("rb_breakout_create: out of host memory"); return RB_ERR_OOM; }
  c->streams = streams; c->history = history; c->max_steps = max_steps; c->seed = seed; c->state = nullptr; c->reset_done = 0;
  if (rb_dev_malloc((void**)&c->state, sizeof(BreakoutStream) * (size_t)streams) != hipSuccess) {
    delete c;
    rb_set_error("rb_breakout_create: device allocation failed");
    return RB_ERR_OOM;
  }
  BreakoutStream init[RB_MAX_STREAMS];
  memset(init, 0, sizeof(init));
  for (int s = 0; s < streams; ++s) init[s].k = 0xFFFFFFFFu;
  const hipError_t e = hipMemcpy(c->state, init, sizeof(BreakoutStream) * (size_t)streams, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    rb_dev_free(c->state);
    delete c;
    rb_set_error("rb_breakout_create: hipMemcpy failed: %s", hipGetErrorString(e));
    return RB_ERR_HIP;
  }
  *out = c;
  return RB_OK;
}

int rb_breakout_destroy(rb_breakout_t* c) {
  if (!c) return RB_OK;
  if (c->state) rb_dev_free(c->state);
  delete c;
  return RB_OK;
}

int rb_breakout_reset(rb_breakout_t* c, float* stacks_dev, rb_stream_t stream) {
  RB_REQUIRE(c && stacks_dev, "rb_breakout_reset: NULL argument");
  RB_REQUIRE(((uintptr_t)stacks_dev & 15u) == 0, "rb_breakout_reset: stacks_dev must be 16-byte aligned");
  RB_LAUNCH(k_breakout_reset, dim3((unsigned)c->streams), dim3(256), stream, c->state, c->seed, (int)c->history, stacks_dev);
  RB_LAUNCH_CHECK();
  c->reset_done = 1;
  return RB_OK;
}

int rb_breakout_step(rb_breakout_t* c, const int32_t* actions_dev, const float* stacks_in_dev, float* stacks_out_dev,
                     float* rewards_dev, uint8_t* nonterminals_dev, int32_t life_terminals, rb_stream_t stream) {
  RB_REQUIRE(c && actions_dev && stacks_in_dev && stacks_out_dev && rewards_dev && nonterminals_dev, "rb_breakout_step: NULL argument");
  RB_REQUIRE((((uintptr_t)stacks_in_dev | (uintptr_t)stacks_out_dev) & 15u) == 0, "rb_breakout_step: the stacks must be 16-byte aligned");
  const size_t bytes = (size_t)c->streams * (size_t)c->history * RB_FRAME_BYTES * sizeof(float);
  const uintptr_t in = (uintptr_t)stacks_in_dev, outp = (uintptr_t)stacks_out_dev;
  RB_REQUIRE(in + bytes <= outp || outp + bytes <= in, "rb_breakout_step: stacks_out_dev overlaps stacks_in_dev (the step is out of place)");
  if (!c->reset_done) {
    rb_set_error("rb_breakout_step: no game in play: call rb_breakout_reset first");
    return RB_ERR_STATE;
  }
  RB_LAUNCH(k_breakout_step, dim3((unsigned)c->streams), dim3(256), stream, c->state, c->seed, (int)c->history, (int)c->max_steps,
            (int)life_terminals, actions_dev, stacks_in_dev, stacks_out_dev, rewards_dev, nonterminals_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

int rb_breakout_get_state(rb_breakout_t* c, rb_breakout_state_t* out_host, rb_stream_t stream) {
  RB_REQUIRE(c && out_host, "rb_breakout_get_state: NULL argument");
  RB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  RB_HIP_TRY(hipMemcpy(out_host, c->state, sizeof(BreakoutStream) * (size_t)c->streams, hipMemcpyDeviceToHost));
  return RB_OK;
}

int rb_breakout_set_state(rb_breakout_t* c, const rb_breakout_state_t* in_host, rb_stream_t stream) {
  RB_REQUIRE(c && in_host, "rb_breakout_set_state: NULL argument");
  for (int s = 0; s < c->streams; ++s) {
    const char* why = rb_brk_invalid_field(in_host[s], c->max_steps);
    RB_REQUIRE(!why, "rb_breakout_set_state: stream %d: %s", s, why);
  }
  RB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  RB_HIP_TRY(hipMemcpy(c->state, in_host, sizeof(BreakoutStream) * (size_t)c->streams, hipMemcpyHostToDevice));
  c->reset_done = 1;
  return RB_OK;
}

int rb_breakout_stats(rb_breakout_t* c, rb_breakout_stats_t* out_host, rb_stream_t stream) {
  RB_REQUIRE(c && out_host, "rb_breakout_stats: NULL argument");
  BreakoutStream host[RB_MAX_STREAMS];
  RB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  RB_HIP_TRY(hipMemcpy(host, c->state, sizeof(BreakoutStream) * (size_t)c->streams, hipMemcpyDeviceToHost));
  out_host->games = 0; out_host->return_sum = 0.0; out_host->bricks = 0; out_host->lives_lost = 0; out_host->steps = 0;
  for (int s = 0; s < c->streams; ++s) {
    out_host->games += host[s].games;
    out_host->return_sum += (double)host[s].return_sum;
    out_host->bricks += host[s].bricks;
    out_host->lives_lost += host[s].lives_lost;
    out_host->steps += host[s].steps;
  }
  return RB_OK;
}

int rb_breakout_reset_stats(rb_breakout_t* c, rb_stream_t stream) {
  RB_REQUIRE(c, "rb_breakout_reset_stats: NULL argument");
  RB_LAUNCH(k_breakout_reset_stats, dim3(1), dim3(64), stream, c->state, (int)c->streams);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

}  // extern "C"
