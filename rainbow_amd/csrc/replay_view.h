// replay_view.h — the validation view: history stacks at given data indices.  Included by replay.hip only.
#pragma once
#include "replay_internal.h"

// ReplayMemory.__next__ (memory.py:167-178): history stack ending at data index i, by one 256-thread workgroup.
// NOTE the reference indexes data[i-h+1 .. i] with numpy negative wrap-around, not % C.
// With S interleaved streams the stack is the slot's own stream: slots i - (h-1-t) S (mod C), t = 0..h-1.
__device__ __forceinline__ void rb_state_stack(const ReplayView& v, int64_t data_index, float* out) {
  __shared__ int s_blank[64];
  const int h = v.history;
  const int64_t S = v.streams;
  if (threadIdx.x == 0) {
    int blank_next = 0;
    s_blank[h - 1] = 0;
    for (int t = h - 2; t >= 0; --t) {
      const int64_t ring_next = rb_floor_mod(data_index - (int64_t)(h - 2 - t) * S, v.capacity);
      const int b = blank_next || (v.timestep[ring_next] == 0);
      s_blank[t] = b;
      blank_next = b;
    }
  }
  __syncthreads();
  for (int t = 0; t < h; ++t) {
    const int64_t ring = rb_floor_mod(data_index - (int64_t)(h - 1 - t) * S, v.capacity);
    const uint8_t* src = v.frames + ring * RB_FRAME_BYTES;
    float* dst = out + (int64_t)t * RB_FRAME_BYTES;
    const bool blank = s_blank[t] != 0;
    for (int p = (int)threadIdx.x; p < RB_FRAME_BYTES; p += (int)blockDim.x)
      dst[p] = blank ? 0.0f : __fdiv_rn((float)src[p], 255.0f);
  }
}

__global__ __launch_bounds__(256) void k_state_at(ReplayView v, int64_t data_index, float* out) {
  rb_state_stack(v, data_index, out);
}

// The same for n data indices at once (one workgroup per state): the validation pass of test.py:38-39 walks the whole
// validation memory — one launch instead of one launch + host loop per state.
__global__ __launch_bounds__(256) void k_states_at(ReplayView v, const int64_t* data_index, float* out) {
  rb_state_stack(v, data_index[blockIdx.x], out + (int64_t)blockIdx.x * v.history * RB_FRAME_BYTES);
}
