// nl_common.h — what every NoisyLinear kernel (model.py:10-46) shares: the weight pointers and the noisy weight itself.
//
// Why a dedicated family (nl_fwd.h, nl_dx.h, nl_dw.h, nl_bwd.h): with M = B..3B rows (32..96) against [1024 x 3136] weights the
// hidden layer is a weight-bandwidth problem — 51 MB of mu/sigma per forward, 26 MB per input-gradient pass, 26 MB of gradient
// written — and each weight is used once per workgroup.  Noisy weights are formed in registers, W = mu + sigma * (eps_out *
// eps_in), with the reference's rounding order (model.py:39,44); eps_w is never materialised.
//
// The 16x16x4 MFMA wants lane l to hold weight row / output column l&15 for k-slot l>>4 and four MFMAs consume one float4 per
// lane (the k permutation inside a step is irrelevant to a sum).  What decides the speed is how many CACHE LINES a wave's load
// instruction touches:
//   * input / weight gradients (output columns contiguous): 16 lanes x 16 B = 256 B per row, 4 rows per instruction = 8 full
//     lines — loaded straight in the operand layout;
//   * forward (k contiguous): the operand layout would be 16 rows x 64 B = 16 half lines per instruction, which measured 31 us
//     against 22 us for the same bytes read as full lines.  The forward therefore loads 8 rows x 128 B per instruction, forms W
//     in that layout and transposes it to the operand layout through a private LDS tile per wave.
//
// Preconditions (checked by the host; the generic gemm_core path remains the fallback):
// K % 32 == 0, all leading dimensions and offsets multiples of 4 floats.
#pragma once
#include "rb_device.h"

struct NlWeights {
  const float* mu;      // [N][K]
  const float* sigma;   // [N][K]
  const float* eout;    // [N]
  const float* ein;     // [streams][K] (offset per row group)
  const float* bmu;     // [N]
  const float* bsigma;  // [N]
};

// W = mu + sigma * (eo * ein): three separately rounded operations
__device__ __forceinline__ float rb_noisy1(float mu, float sg, float eo, float e) { return mu + sg * (eo * e); }
__device__ __forceinline__ float4 rb_noisy4(float4 mu, float4 sg, float eo, float4 e) {
  float4 w;
  w.x = rb_noisy1(mu.x, sg.x, eo, e.x);
  w.y = rb_noisy1(mu.y, sg.y, eo, e.y);
  w.z = rb_noisy1(mu.z, sg.z, eo, e.z);
  w.w = rb_noisy1(mu.w, sg.w, eo, e.w);
  return w;
}
// ... and its adjoint: g_sigma = g_mu * (eo * ein), the same product of the two noise factors first (model.py:39,44)
__device__ __forceinline__ float4 rb_noisy_grad4(float4 gm, float eo, float4 e) {
  float4 gs;
  gs.x = gm.x * (eo * e.x); gs.y = gm.y * (eo * e.y); gs.z = gm.z * (eo * e.z); gs.w = gm.w * (eo * e.w);
  return gs;
}

// Which layer a backward launch works on — 0 the output layer, 1 the hidden layer — for the RB_STAMP builds, which give the two
// launches timeline ids 8 + layer and span slots from 3 * layer: the hidden layer reduces over the flattened conv output (K in
// the thousands), the output layer over the hidden units.
__device__ __forceinline__ int rb_nl_layer(int K) { return K > 1000 ? 1 : 0; }
