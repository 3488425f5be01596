// frames.hip — the observation front end on the device: raw emulator screens to the 84 x 84 unit-range frames the actor and
// the replay consume (rb_frame_preprocess, rb_u8_to_unit_f32), and the S-stream frame-stack step (obs_stack.h).
#include "obs_stack.h"   // rb_resize_tap / rb_resize_pixel, and the S-stream frame-stack front end (rb_obs_stack_step)

// ---------------------------------------------------------------- frame pipeline --
// env.py:27-29 (cv2.resize(gray [H][W] u8, (84, 84), INTER_LINEAR) -> f32 / 255) and env.py:57-69 (element-wise max over the
// last two frames of the action repeat) on the device: raw emulator screens in, the observation the actor and
// ReplayMemory.append consume out — no host-side resize, no 28 KB H2D float frame per environment step.
// The resize is OpenCV's 8-bit fixed-point INTER_LINEAR (11-bit coefficients; oracle/frame_oracle.py has the algebra and
// says why this row is parity-UNPINNED: cv2 is absent here).  One thread per output pixel; the taps of a pixel are four
// bytes per frame, the coefficients two float operations — nothing worth staging.
__global__ __launch_bounds__(256) void k_frame_preprocess(const uint8_t* a, const uint8_t* b, int H, int W, int n_pairs,
                                                           int64_t pair_stride, float* out) {
  const int pair = (int)blockIdx.y;
  const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= 84 * 84 || pair >= n_pairs) return;
  const int dy = p / 84, dx = p - dy * 84;
  int sx, a0, a1, sy, b0, b1;
  rb_resize_tap(dx, 84, W, true, &sx, &a0, &a1);
  rb_resize_tap(dy, 84, H, false, &sy, &b0, &b1);
  int v = rb_resize_pixel(a + pair * pair_stride, H, W, sx, a0, a1, sy, b0, b1);
  if (b) {
    const int w = rb_resize_pixel(b + pair * pair_stride, H, W, sx, a0, a1, sy, b0, b1);
    v = w > v ? w : v;                               // max of the two states == state of the max (x / 255 is monotone)
  }
  out[(int64_t)pair * 84 * 84 + p] = __fdiv_rn((float)(v & 0xFF), 255.0f);    // torch .div_(255)
}

__global__ __launch_bounds__(256) void k_u8_to_unit(const uint8_t* src, float* dst, int64_t n) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
    dst[t] = __fdiv_rn((float)src[t], 255.0f);  // memory.py:137 .div_(255)
}

extern "C" {

int rb_frame_preprocess(const uint8_t* frame_a_dev, const uint8_t* frame_b_dev, int32_t height, int32_t width, int32_t n,
                        float* out_dev, rb_stream_t stream) {
  RB_REQUIRE(frame_a_dev && out_dev, "rb_frame_preprocess: NULL argument");
  RB_REQUIRE(height >= 2 && width >= 2 && height <= 4096 && width <= 4096, "rb_frame_preprocess: frame size must be in [2, 4096]^2");
  RB_REQUIRE(n >= 0, "rb_frame_preprocess: n must be >= 0");
  if (n == 0) return RB_OK;
  RB_LAUNCH(k_frame_preprocess, dim3((unsigned)rb_div_up(84 * 84, 256), (unsigned)n), dim3(256), stream, frame_a_dev, frame_b_dev,
            height, width, n, (int64_t)height * width, out_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

int rb_u8_to_unit_f32(const uint8_t* src_dev, float* dst_dev, int64_t n, rb_stream_t stream) {
  RB_REQUIRE(src_dev && dst_dev && n >= 0, "rb_u8_to_unit_f32: bad argument");
  if (n == 0) return RB_OK;
  int64_t g = rb_div_up(n, 256);
  if (g > 4096) g = 4096;
  RB_LAUNCH(k_u8_to_unit, dim3((unsigned)g), dim3(256), stream, src_dev, dst_dev, n);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

}  // extern "C"
