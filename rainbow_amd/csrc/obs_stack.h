// obs_stack.h — the observation front end of S host emulators on the device (included by frames.hip; the rules are in
// include/rainbow_hip.h).
//
// env.py's wrapper around the emulator, for all S streams in ONE launch per round: the 84 x 84 resize of the raw u8 screens
// (env.py:27-29), the max over the last two frames of the action repeat (env.py:56-67, either or both may be missing when the
// repeat was cut), the state deque (env.py:24,68,77) and its blanking at a true reset (env.py:31-33,41).  The launch is
// latency-bound (S x history frames of 28 KB), so the work is split finer than one workgroup per stream: grid (frame chunk,
// history slot, stream), one 16-byte lane per thread.  The threads of the newest slot compute four adjacent output pixels,
// which lie in one row (84 = 4 x 21) and share its vertical taps.  Stateless: the caller owns both stack buffers.
#pragma once
#include "rb_common.h"

#include <string.h>

// ---- OpenCV's 8-bit fixed-point INTER_LINEAR (11-bit coefficients; oracle/frame_oracle.py has the algebra and says why this
// row is parity-UNPINNED: cv2 is absent here).  Shared by k_frame_preprocess (frames.hip) and k_obs_stack.
__device__ __forceinline__ void rb_resize_tap(int d, int dst, int src, bool clamp_f, int* s_out, int* c0, int* c1) {
  const double scale = (double)src / (double)dst;
  float f = (float)__dsub_rn(__dmul_rn((double)d + 0.5, scale), 0.5);          // float((d + 0.5) * scale - 0.5)
  int s = (int)floorf(f);
  f = __fsub_rn(f, (float)s);
  if (clamp_f) {
    if (s < 0) { f = 0.0f; s = 0; }
    if (s >= src - 1) { f = 0.0f; s = src - 1; }
  }
  *s_out = s;
  *c0 = __float2int_rn(__fmul_rn(__fsub_rn(1.0f, f), 2048.0f));               // saturate_cast<short>(cbuf * INTER_RESIZE_COEF_SCALE)
  *c1 = __float2int_rn(__fmul_rn(f, 2048.0f));
}
__device__ __forceinline__ int rb_resize_pixel(const uint8_t* img, int H, int W, int sx, int a0, int a1, int sy, int b0, int b1) {
  const int x1 = sx + 1 < W ? sx + 1 : W - 1;
  const int y0 = sy < 0 ? 0 : (sy > H - 1 ? H - 1 : sy);
  const int y1 = sy + 1 < 0 ? 0 : (sy + 1 > H - 1 ? H - 1 : sy + 1);
  const int h0 = (int)img[(int64_t)y0 * W + sx] * a0 + (int)img[(int64_t)y0 * W + x1] * a1;
  const int h1 = (int)img[(int64_t)y1 * W + sx] * a0 + (int)img[(int64_t)y1 * W + x1] * a1;
  return ((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16)) + 2) >> 2;
}

#define RB_OBS_MAX_HISTORY 16
#define RB_OBS_LANES (RB_FRAME_BYTES / 4)     // 16-byte lanes of one float32 frame: 1764 = 84 rows x 21

struct ObsFlags {
  uint8_t f[RB_MAX_STREAMS];                  // by value in the argument block, as the scalars of k_append_streams
};

__global__ __launch_bounds__(256) void k_obs_stack(const uint8_t* a, const uint8_t* b, int H, int W, int history, ObsFlags fl,
                                                    const float* stacks_in, float* stacks_out) {
  const int w = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (w >= RB_OBS_LANES) return;
  const int slot = (int)blockIdx.y, s = (int)blockIdx.z;
  const int flags = (int)fl.f[s];
  float4* dst = (float4*)(stacks_out + ((int64_t)s * history + slot) * RB_FRAME_BYTES) + w;
  if (slot < history - 1) {                   // env.py:68 (deque append drops the oldest) / env.py:31-33 (blank fill)
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!(flags & RB_OBS_BLANK)) v = ((const float4*)(stacks_in + ((int64_t)s * history + slot + 1) * RB_FRAME_BYTES))[w];
    *dst = v;
    return;
  }
  const bool has_a = (flags & RB_OBS_FRAME_A) != 0, has_b = (flags & RB_OBS_FRAME_B) != 0;
  int px[4] = {0, 0, 0, 0};                   // env.py:56: a frame the repeat never took stays zero
  if (has_a || has_b) {
    const int dy = w / 21, dx0 = 4 * (w - dy * 21);
    const int64_t screen = (int64_t)s * H * W;
    int sy, b0, b1;
    rb_resize_tap(dy, 84, H, false, &sy, &b0, &b1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int sx, a0, a1;
      rb_resize_tap(dx0 + j, 84, W, true, &sx, &a0, &a1);
      int v = 0;
      if (has_a) v = rb_resize_pixel(a + screen, H, W, sx, a0, a1, sy, b0, b1);
      if (has_b) {
        const int u = rb_resize_pixel(b + screen, H, W, sx, a0, a1, sy, b0, b1);
        v = u > v ? u : v;                    // max of the two states == state of the max (x / 255 is monotone)
      }
      px[j] = v;
    }
  }
  *dst = make_float4(__fdiv_rn((float)(px[0] & 0xFF), 255.0f), __fdiv_rn((float)(px[1] & 0xFF), 255.0f),
                     __fdiv_rn((float)(px[2] & 0xFF), 255.0f), __fdiv_rn((float)(px[3] & 0xFF), 255.0f));   // torch .div_(255)
}

extern "C" {

int rb_obs_stack_step(const uint8_t* frames_a_dev, const uint8_t* frames_b_dev, int32_t height, int32_t width, int32_t streams,
                      int32_t history, const uint8_t* flags_host, const float* stacks_in_dev, float* stacks_out_dev,
                      rb_stream_t stream) {
  RB_REQUIRE(stacks_in_dev, "rb_obs_stack_step: stacks_in_dev is NULL");
  RB_REQUIRE(stacks_out_dev, "rb_obs_stack_step: stacks_out_dev is NULL");
  RB_REQUIRE(flags_host, "rb_obs_stack_step: flags_host is NULL");
  RB_REQUIRE(((uintptr_t)stacks_in_dev & 15u) == 0, "rb_obs_stack_step: stacks_in_dev must be 16-byte aligned");
  RB_REQUIRE(((uintptr_t)stacks_out_dev & 15u) == 0, "rb_obs_stack_step: stacks_out_dev must be 16-byte aligned");
  RB_REQUIRE(streams >= 1 && streams <= RB_MAX_STREAMS, "rb_obs_stack_step: streams must be in [1, %d], got %d", RB_MAX_STREAMS,
             (int)streams);
  RB_REQUIRE(history >= 1 && history <= RB_OBS_MAX_HISTORY, "rb_obs_stack_step: history must be in [1, %d], got %d",
             RB_OBS_MAX_HISTORY, (int)history);
  RB_REQUIRE(height >= 2 && height <= 4096, "rb_obs_stack_step: height must be in [2, 4096], got %d", (int)height);
  RB_REQUIRE(width >= 2 && width <= 4096, "rb_obs_stack_step: width must be in [2, 4096], got %d", (int)width);
  const size_t bytes = (size_t)streams * (size_t)history * RB_FRAME_BYTES * sizeof(float);
  const uintptr_t in = (uintptr_t)stacks_in_dev, outp = (uintptr_t)stacks_out_dev;
  RB_REQUIRE(in + bytes <= outp || outp + bytes <= in,
             "rb_obs_stack_step: stacks_out_dev overlaps stacks_in_dev (the step is out of place)");
  ObsFlags fl;
  memset(&fl, 0, sizeof(fl));
  for (int s = 0; s < streams; ++s) {         // by value: the caller's array is free again when this returns
    const int f = flags_host[s];
    RB_REQUIRE(f <= (RB_OBS_BLANK | RB_OBS_FRAME_A | RB_OBS_FRAME_B), "rb_obs_stack_step: flags_host[%d] = %d is above 7", s, f);
    RB_REQUIRE(!(f & RB_OBS_FRAME_A) || frames_a_dev, "rb_obs_stack_step: flags_host[%d] has FRAME_A but frames_a_dev is NULL", s);
    RB_REQUIRE(!(f & RB_OBS_FRAME_B) || frames_b_dev, "rb_obs_stack_step: flags_host[%d] has FRAME_B but frames_b_dev is NULL", s);
    fl.f[s] = (uint8_t)f;
  }
  RB_LAUNCH(k_obs_stack, dim3((unsigned)rb_div_up(RB_OBS_LANES, 256), (unsigned)history, (unsigned)streams), dim3(256), stream,
            frames_a_dev, frames_b_dev, (int)height, (int)width, (int)history, fl, stacks_in_dev, stacks_out_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

}  // extern "C"
