// conv_fwd.h — the forward convolution kernels with LDS-resident operands (model.py:56-58,61-62).  This header holds what the host
// and the launch plan need of them (the argument struct, the output store, the LDS and wave sizing) and includes the kernels:
//   conv_fwd_t16.h    the whole-K 16x16x4 tile pieces more than one kernel uses: lane setup, bias fetch, epilogue, half-unit exchange
//                     (the tile's MFMA steps are rb_t16_steps of conv_stage.h)
//   conv_fwd_image.h  rb_conv_fwd_body, one image per workgroup (32x32x2 tiles with the reduction split over 8 waves, or whole-K
//                     16x16x4 tiles), behind k_conv_fwd_lds and k_conv_fwd_t16
//   conv_fwd_multi.h  k_conv_fwd_multi_t16, the image loop around the t16 tile (later layers, large batches)
//   conv_fwd_full.h   k_conv_fwd_full, whole image per workgroup (first layer, large batches), and its sizing ConvFwdFullLds
// Included by learner_internal.h.
//
// At batch 32 the Rainbow conv stack is tiny per image (28 KB of u8 input, <= 51 KB activations,
// <= 147 KB of weights per layer) and the generic implicit GEMM of gemm_core.h spends its time on
// per-element im2col address arithmetic and dependent global loads, not on MFMAs.  Here a
// workgroup stages what it needs ONCE with wide coalesced loads —
//     the input patch of its output positions (u8 frames decoded to exact x/255 on the way in),
//     a 32-channel slab of the weights, transposed to [k][32] so MFMA operand reads are
//     bank-conflict free,
//     a k -> patch-offset table (no div/mod in the inner loop),
// — and then runs a pure LDS -> v_mfma_f32_32x32x2_f32 loop.  The four waves split K; their
// accumulators are reduced through LDS in a fixed order (deterministic) and the epilogue (bias,
// ReLU / ReLU mask) stores rows that are contiguous in the NCHW activation.
#pragma once
#include "conv_stage.h"
#include "kernel_stamp.h"

struct ConvLdsFwdArgs {
  int cin, cout;
  int n_on;                  // images [0,n_on) use net 0, the rest net 1
  const float* w[2];         // [cout][cin*KK]
  const float* bias[2];
  ImgSrc src;                // FIRST layer input
  const float* in_f;         // later layers: [img][cin][IP]
  float* out;                // [img][cout][P]
  float* out_blocked;        // optional second copy of the flattened output in the k-blocked layout of nl_fwd.h
  int rows_total;            //   ... with this many rows (images)
  int ipb;                   // k_conv_fwd_multi_t16 / k_conv_fwd_full: images per workgroup
  // grid = (images or image groups, cout tiles, position chunks) instead of (position chunks, cout tiles, images or groups):
  // workgroups are spread over the 8 XCDs by linear block index mod 8; with the image as the fastest index (and an
  // image count that is a multiple of 8) every workgroup of image i, in every layer, runs on XCD i mod 8 — the next layer's
  // input is then in that XCD's own L2 instead of behind the fabric
  int img_fast;
};

// one output element (image img, channel m, position p) of a forward epilogue: the NCHW activation and, where asked for, its
// k-blocked copy
template <class G>
__device__ __forceinline__ void rb_conv_store_out(const ConvLdsFwdArgs& a, int img, int m, int p, float o) {
  a.out[((int64_t)img * a.cout + m) * G::P + p] = o;
  if (a.out_blocked) a.out_blocked[rb_blocked_index(img, m * G::P + p, a.rows_total)] = o;   // x.view(-1, conv_output_size), model.py:71
}

// ---- sizing of the one-image and image-loop kernels: LDS floats and waves per workgroup --------------------------------------------
// PR = input rows staged per channel (covers the output rows of one position chunk).
// PCH = output positions per workgroup (<= 32 NT; a multiple of the row length keeps the patch at PR rows).
// T16 (the whole-K 16x16x4 tile kernels): no reduction scratch, no tap table; the channel planes of the patch are padded (ConvPatch)
// so that the four k-slots of a 16x16x4 operand read (channel groups cin/4 apart) start 16 banks apart.
template <class G, int KMAX, int PLANE, int RP, int SUB>
__device__ __forceinline__ constexpr int rb_t16_off(int j) {            // step j of a lane's K quarter -> offset in the patch
  return (j / G::KK) * PLANE + ((j % G::KK) / G::KS) * RP + (((j % G::KK) % G::KS) % G::S) * SUB + ((j % G::KK) % G::KS) / G::S;
}
template <class G, int PR, int KMAX, bool T16 = false>
struct ConvFwdLdsSize {
  static constexpr int KGRAN = 2 * RB_CONV_WAVES;
  static constexpr int KPAD = (KMAX + KGRAN - 1) / KGRAN * KGRAN;
  static constexpr int RED = RB_CONV_WAVES * 16 * 64;      // reduction scratch (floats) for ONE 32-position tile, overlays the operands
  // the weight slab keeps its GLOBAL orientation in LDS: 32 rows (output channels) of KPAD + 4 floats.  Staging is then
  // 16-byte loads -> 16-byte LDS stores, conflict-free (a [k][33] transposed image took 16 scalar stores per
  // thread at 8-way bank conflicts: 1-1.5 us of every workgroup, and it serialised the two first-layer workgroups of a CU —
  // tools/wg_timeline.py: 5.3 us input stage for the second one); the MFMA operand read (lane = row) is 4-way conflicted
  // instead, one read per NT MFMAs, hidden under them.
  static constexpr int WS = KPAD + 4;
  static constexpr int CQ = (KMAX / G::KK) / 4;            // T16: channels per k-slot
  typedef ConvPatch<G, PR, T16 ? CQ : 0> PG;               // the patch: de-interleaved rows, T16: padded planes
  static constexpr int SUB = PG::SUB, RP = PG::RP, PLANE = PG::PLANE;
  static __device__ __forceinline__ constexpr int at(int j) { return rb_t16_off<G, KMAX, PLANE, RP, SUB>(j); }   // rb_t16_steps
  static constexpr int OPS = 32 * WS + (KMAX / G::KK) * PLANE;       // weights then patch, contiguous
  static constexpr int WSZ = T16 ? OPS : (OPS > RED ? OPS : RED);
  static constexpr int FLOATS = WSZ + (T16 ? 0 : KPAD);    // + the tap table (ints)
};
// T16: the workgroup has one wave per 16-position x 16-channel output tile (PT position tiles x 2 channel tiles), every wave runs
// the WHOLE K for its tile (conv_fwd_image.h); otherwise the 8 waves split the reduction.
template <int KMAX, int PCH, bool T16>
struct ConvFwdWaves {
  static constexpr int PT = (PCH + 15) / 16;
  // The wave count is rounded up to a multiple of 4 — an even share per SIMD: a 10-wave workgroup
  // puts 3 waves on two SIMDs, and the compiler, which sizes the register allocation for the AVERAGE waves per SIMD its LDS
  // footprint allows (next_free_vgpr is raised to the smallest count that still gives that occupancy), then leaves no room
  // for the second workgroup the LDS would admit (profiles/round4_experiments.txt §5); the spare waves help staging and leave
  // SPLIT_LAST (a wave per (position tile, channel tile) unit, 2 PT = 4 n + 2 units: the first layer's 80-position chunks, ten
  // units): waves w, w + 4, w + 8 share a SIMD, so two SIMDs multiplied for three units and two for two — and with two such
  // workgroups per CU those SIMDs' MFMAs were the launch's critical path.  The last two units run instead as four half-units
  // (unit, reduction half) on four waves, one per SIMD; the halves meet through 4 KB of LDS: 2.5 units per SIMD.
  static constexpr bool SPLIT_LAST = T16 && PT >= 3 && ((2 * PT) % 4) == 2 && ((KMAX / 4) % 8) == 0;
  static constexpr int TILE_WAVES = T16 ? (SPLIT_LAST ? 2 * PT + 2 : 2 * PT) : PT;
  static constexpr int PARTF = SPLIT_LAST ? 4 * 4 * 64 : 0;   // floats of LDS behind ConvFwdLdsSize::FLOATS for the half-units' partial tiles
  static constexpr int NWV = T16 ? (TILE_WAVES + 3) / 4 * 4 : RB_CONV_WAVES;
};

#include "conv_fwd_t16.h"
#include "conv_fwd_image.h"
#include "conv_fwd_multi.h"
#include "conv_fwd_full.h"
