// replay_shift.h — the frame-stack gather with random-shift augmentation (DrQ: pad the 84 x 84 stack by `pad` pixels of edge
// replication, crop 84 x 84 at a random offset): k_gather_stacks_shift.  Included by replay.hip only, after replay_sample.h
// (the plain gather, k_gather_stacks, whose pad = 0 case this one reproduces byte for byte).
#pragma once
#include "replay_internal.h"

#define RB_SHIFT_MAX_PAD 8
#define RB_SHIFT_KEY_TAG 0x5348494654ull      // "SHIFT": keeps these draws off the sampler's stream (key = seed, replay_sample.h)
#define RB_FRAME_SIDE 84
#define RB_FRAME_ROW_DWORDS (RB_FRAME_SIDE / 4)
#define RB_FRAME_DWORDS (RB_FRAME_BYTES / 4)

// one value of a Philox word in [-pad, pad]: the high word of v (2 pad + 1), no modulo bias beyond 2^-32
__device__ __forceinline__ int rb_shift_from_u32(uint32_t v, int pad) {
  return (int)(((uint64_t)v * (uint64_t)(2 * pad + 1)) >> 32) - pad;
}

// block = (sample i, stack w in {state, next}, frame c): the source frame goes into LDS once (441 sixteen-byte loads, as in
// k_gather_stacks) and every OUTPUT dword is built from there — a row is 84 B = 21 dwords, so an output dword never straddles
// two source rows:  out[y][x] = frame[clamp(y + dy)][clamp(x + dx)], clamp onto [0, 83].
//   interior dword (source columns 4q + dx .. 4q + dx + 3 all inside the row): two adjacent LDS dwords, byte-aligned by
//   (4q + dx) & 3 (rb_alignbyte); when the alignment is 0 and the dword is the row's last, the second operand is the first dword
//   of the next row — or, in the last row, the pad dword behind the frame — and contributes no byte;
//   edge dwords (at most ceil(pad / 4) + 1 per row side): four clamped byte picks out of LDS dwords.
// (dy, dx) is shared by the `history` frames of one (i, w): injected (shifts_in, int8 [B][2][2] = [i][w] -> (dy, dx), clamped to
// [-pad, pad]) or Philox4x32-10 with key seed ^ RB_SHIFT_KEY_TAG and counter (hi = draw, lo = i): words 0, 1 = the state's
// (dy, dx), words 2, 3 = the next state's.  The header (its rng_counter included) is not touched.
__global__ __launch_bounds__(256) void k_gather_stacks_shift(ReplayView v, int32_t batch, const int32_t* win, int32_t win_stride, int32_t pad,
                                                              uint64_t key, uint64_t draw, const int8_t* shifts_in,
                                                              uint8_t* states, uint8_t* next_states, int8_t* shifts_out) {
  constexpr int VEC = RB_FRAME_BYTES / 16;
  __shared__ __attribute__((aligned(16))) uint32_t s_frame[RB_FRAME_DWORDS + 4];    // + the pad dword (a whole 16-byte slot)
  const int h = v.history, n = v.n;
  const int per_sample = 2 * h;
  const int b = (int)blockIdx.x;
  if (b >= batch * per_sample) return;                                 // block-uniform
  const int i = b / per_sample;
  const int s = b % per_sample;
  const int w = s >= h ? 1 : 0;
  const int c = w ? s - h : s;
  const int slot = w ? n + c : c;
  int dy, dx;
  if (shifts_in) {
    dy = (int)shifts_in[(i * 2 + w) * 2 + 0];
    dx = (int)shifts_in[(i * 2 + w) * 2 + 1];
    dy = dy < -pad ? -pad : (dy > pad ? pad : dy);
    dx = dx < -pad ? -pad : (dx > pad ? pad : dx);
  } else {
    const rb_philox_out r = rb_philox(key, draw, (uint64_t)i);
    dy = rb_shift_from_u32(r.v[2 * w + 0], pad);
    dx = rb_shift_from_u32(r.v[2 * w + 1], pad);
  }
  if (shifts_out && c == 0 && threadIdx.x == 0) {
    shifts_out[(i * 2 + w) * 2 + 0] = (int8_t)dy;
    shifts_out[(i * 2 + w) * 2 + 1] = (int8_t)dx;
  }
  const int32_t ring = win[(int64_t)i * win_stride + slot];
  uint4* d = (uint4*)((w ? next_states : states) + ((int64_t)i * h + c) * RB_FRAME_BYTES);
  if (ring < 0) {                                                      // block-uniform: a blanked slot stays blank
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (int t = (int)threadIdx.x; t < VEC; t += (int)blockDim.x) d[t] = z;
    return;
  }
  const uint4* src = (const uint4*)(v.frames + (int64_t)ring * RB_FRAME_BYTES);
  uint4* s4 = (uint4*)s_frame;
  for (int t = (int)threadIdx.x; t < VEC; t += (int)blockDim.x) s4[t] = src[t];
  if (threadIdx.x == 0) s_frame[RB_FRAME_DWORDS] = 0u;                 // the pad dword: read (alignment 0), never used
  __syncthreads();
  auto clampi = [](int x) { return x < 0 ? 0 : (x > RB_FRAME_SIDE - 1 ? RB_FRAME_SIDE - 1 : x); };
  for (int t = (int)threadIdx.x; t < VEC; t += (int)blockDim.x) {
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int od = 4 * t + k;                                        // output dword 0 .. 1763
      const int y = od / RB_FRAME_ROW_DWORDS, q = od - y * RB_FRAME_ROW_DWORDS;
      const int row = clampi(y + dy) * RB_FRAME_ROW_DWORDS;            // first LDS dword of the source row
      const int sx = 4 * q + dx;                                       // source column of the dword's byte 0
      if (sx >= 0 && sx + 3 <= RB_FRAME_SIDE - 1) {
        const int j = row + (sx >> 2);                                 // j + 1 <= 1764: inside the padded array
        o[k] = rb_alignbyte(s_frame[j + 1], s_frame[j], (unsigned)(sx & 3));
      } else {
        uint32_t acc = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = clampi(sx + e);
          acc |= ((s_frame[row + (col >> 2)] >> (8 * (col & 3))) & 0xffu) << (8 * e);
        }
        o[k] = acc;
      }
    }
    d[t] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}
