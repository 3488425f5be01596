// nl_bwd.h — the fused backward launch of one NoisyLinear layer.  Horizontal fusion: the weight gradient (nl_dw.h) and the input
// gradient (nl_dx.h) of a layer are independent given dY, so both run in ONE launch (one ~5 us kernel boundary less on the
// critical path).  Blocks [0, dw_x*dw_y) take the dW tiles, the rest the dX tiles; the output layer's launch can carry the
// replay's priority write-back as a third tenant (the only reason this header needs replay_internal.h).
#pragma once
#include "nl_dx.h"
#include "nl_dw.h"
#include "kernel_stamp.h"
#include "replay_internal.h"

// the input-gradient body of a launch: rb_nl_dx_body<4, 4> | <2, 8> (batch <= 32) | <4, 8>; k_nl_bwd<TALL>: rb_nl_dx_body_tall
enum NlDxBody { RB_NL_DX_M64_ST4, RB_NL_DX_M32_ST8, RB_NL_DX_M64_ST8, RB_NL_DX_TALL };
struct NlBwdGrid { int dw_x, dw_y, dx_x, dx_y, dx_z; int dx_body; };
// Optional third tenant of the output layer's backward launch: the sum-tree priority write-back (agent.py:100,
// memory.py:157-159).  It depends only on (tree indices, per-sample loss), both final before this launch, and is a
// single-workgroup latency chain — as one more block here it costs nothing on the step's critical path.
struct NlPriorityUpdate {
  int enabled;               // 0 / 1
  ReplayView view;
  const int64_t* tree_idx;
  const float* loss;
  int n;
  double omega;
  // the early draw (replay_internal.h rb_replay_spec_launch; enabled == 0): this launch is the first one behind the head kernel,
  // so its START proves the per-sample losses final — workgroup 0 stores go_epoch for the replay's stream to see (NULL: nothing)
  unsigned* go_flag;
  unsigned go_epoch;
};
// TALL: 512-thread workgroups whose input-gradient blocks run rb_nl_dx_body_tall (the output layer at batch <= 32: 40
// workgroups, LDS and occupancy are no concern); its weight-gradient blocks use the first four waves, the others leave.
template <bool TALL>
__global__ __launch_bounds__(TALL ? 64 * RB_NL_DXT_WAVES : 256) void k_nl_bwd(NlDwArgs dw, NlDxArgs dx, NlBwdGrid g, NlPriorityUpdate up) {
  // ONE LDS buffer for whichever body this workgroup runs (separate static arrays would add up: 132 KB, one workgroup
  // per CU for the whole launch; 32 KB lets five share a CU)
  constexpr int LDS0 = RB_NL_DX_LDS > UpdateLds<512, 256>::WORDS ? RB_NL_DX_LDS : UpdateLds<512, 256>::WORDS;
  constexpr int LDSW = TALL ? (RB_NL_DXT_LDS > LDS0 ? RB_NL_DXT_LDS : LDS0) : LDS0;
  __shared__ __attribute__((aligned(16))) float lds[LDSW];
  // the write-back block goes FIRST: it is the launch's longest single-workgroup chain and must not queue behind the tiles
  int b = (int)blockIdx.x;
  // RB_STAMP builds: span slots 0-2 / 3-5 of the output / hidden layer's launch, and the per-workgroup timeline
  // (tools/nl_timeline.py): kernel id 8 = output layer's launch, 9 = hidden layer's; slot 0 start, 1 role (0 write-back, 1 dW,
  // 2 dX), 6 end, 7 where it ran
  const int layer = rb_nl_layer(dw.K);
  const int sb = 3 * layer, kid = 8 + layer, wgb = (int)blockIdx.x;
  (void)sb; (void)kid; (void)wgb;
  RB_WGT(kid, wgb, 0);
  RB_WGT_HW(kid, wgb);
  if (up.go_flag && blockIdx.x == 0 && threadIdx.x == 0) {
#if defined(RB_HOST_INTERP)
    *up.go_flag = up.go_epoch;
#else
    __hip_atomic_store(up.go_flag, up.go_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
  }
  if (up.enabled) {
    if (TALL && threadIdx.x >= 256 && b == 0) return;    // (the write-back body is written for 256 threads)
    if (b == 0) {
      RB_SPAN_BEGIN(sb + 0);
      // a sorted batch of <= 64 leaves — what the sampler hands back — on ONE wave without LDS tables or workgroup barriers
      // (rb_update_sorted_wave), anything else through the hashed body (17.0 us and this launch's pole, round6_final_wg_timeline_b32.txt).
      // Same tree, bit for bit, either way.
      rb_update_auto<512, 256>(up.view, up.tree_idx, up.loss, up.n, 1, up.omega, lds);     // n <= 256
      RB_SPAN_END(sb + 0);
      RB_WGT_ROLE(kid, wgb, 0);
      RB_WGT(kid, wgb, 6);
      return;
    }
    b -= 1;
  }
  const int ndw = g.dw_x * g.dw_y;
  if (b < ndw) {
    if (TALL && threadIdx.x >= 256) return;              // the weight-gradient bodies are 4-wave bodies
    RB_SPAN_BEGIN(sb + 1);
    if (dw.ct == 4) rb_nl_dw_body_pipe_all<4>(dw, b % g.dw_x, b / g.dw_x, 4 * b);     // block-uniform
    else if (dw.ct > 0) rb_nl_dw_body_pipe(dw, b % g.dw_x, b / g.dw_x, 4 * b);
    else rb_nl_dw_body(dw, b % g.dw_x, b / g.dw_x, 4 * b);
    RB_SPAN_END(sb + 1);
    RB_WGT_ROLE(kid, wgb, 1);
  } else {
    const int r = b - ndw;
    RB_SPAN_BEGIN(sb + 2);
    if constexpr (TALL) {
      rb_nl_dx_body_tall(dx, r % g.dx_x, r / g.dx_x, lds);
    }
    else if (g.dx_body == RB_NL_DX_M64_ST8) rb_nl_dx_body<4, 8>(dx, r % g.dx_x, (r / g.dx_x) % g.dx_y, r / (g.dx_x * g.dx_y), lds);   // block-uniform
    else if (g.dx_body == RB_NL_DX_M32_ST8) rb_nl_dx_body<2, 8>(dx, r % g.dx_x, (r / g.dx_x) % g.dx_y, r / (g.dx_x * g.dx_y), lds);
    else rb_nl_dx_body<4, 4>(dx, r % g.dx_x, (r / g.dx_x) % g.dx_y, r / (g.dx_x * g.dx_y), lds);
    RB_SPAN_END(sb + 2);
    RB_WGT_ROLE(kid, wgb, 2);
  }
  RB_WGT(kid, wgb, 6);
}
