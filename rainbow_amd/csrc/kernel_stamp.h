// kernel_stamp.h — the in-kernel timestamps of the RB_STAMP / RB_STAMP_FINE diagnostic builds (tools/build_variant.sh): RB_CSTAMP
// (one slot per phase of a launch's first / last workgroup, g_cstamp; RB_FSTAMP: k_conv_fwd_full's slots of it), RB_WGT (the
// per-workgroup timeline, g_wgt) and RB_SPAN (the span of a launch's tenants, g_span); in the product build every macro is
// ((void)0).  learner.hip defines the three arrays and reads them back.  Included directly by every header whose kernels stamp:
// conv_fwd.h (for its sections conv_fwd_image.h, conv_fwd_multi.h and conv_fwd_full.h), conv_dx.h, conv_dw.h, fc_gemm.h, nl_dx.h,
// nl_bwd.h, head.h, act_path.h (whose bodies in act_conv.h, act_fc.h and act_head.h do not stamp), and by learner.hip.
#pragma once
#include "rb_device.h"

#if defined(RB_STAMP)
extern __device__ long long g_cstamp[64];
#define RB_CSTAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) g_cstamp[i] = wall_clock64(); } while (0)
#define RB_CSTAMP_LAST(i) do { if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1 && blockIdx.y == gridDim.y - 1 && blockIdx.z == gridDim.z - 1) g_cstamp[i] = wall_clock64(); } while (0)
// k_conv_fwd_full's slots (tools/stamp/fstamp.py): `on` is the kernel's own flag for the one thread that stamps
#define RB_FSTAMP(on, i) do { if (on) g_cstamp[i] = wall_clock64(); } while (0)
// per-workgroup timeline: g_wgt[kernel id][workgroup][slot] = wall_clock64 (100 MHz) at phase boundaries, slot 7 = where
// it ran (XCC id << 16 | HW_ID bits) — tools/wg_timeline.py draws the schedule of a launch from it
#define RB_WGT_KERNELS 14
#define RB_WGT_WGS 2048
extern __device__ long long g_wgt[RB_WGT_KERNELS][RB_WGT_WGS][8];
#define RB_WGT(kid, wg, slot) do { if (threadIdx.x == 0 && (wg) < RB_WGT_WGS) g_wgt[kid][wg][slot] = wall_clock64(); } while (0)
#define RB_WGT_HW(kid, wg) do { if (threadIdx.x == 0 && (wg) < RB_WGT_WGS) g_wgt[kid][wg][7] = ((long long)__builtin_amdgcn_s_getreg(6164) << 16) | (__builtin_amdgcn_s_getreg(63492) & 0xffff); } while (0)
#define RB_WGT_ROLE(kid, wg, role) do { if (threadIdx.x == 0 && (wg) < RB_WGT_WGS) g_wgt[kid][wg][1] = (role); } while (0)
// spans of a launch's tenants: g_span[2 * slot] = earliest start, [2 * slot + 1] = latest end of the blocks that ran `slot` since
// the host last reset the array (tools/stamp/span.py)
extern __device__ long long g_span[64];
#define RB_SPAN_BEGIN(slot) do { if (threadIdx.x == 0) atomicMin((unsigned long long*)&g_span[2 * (slot)], (unsigned long long)wall_clock64()); } while (0)
#define RB_SPAN_END(slot) do { __syncthreads(); if (threadIdx.x == 0) atomicMax((unsigned long long*)&g_span[2 * (slot) + 1], (unsigned long long)wall_clock64()); } while (0)
#else
#define RB_SPAN_BEGIN(slot) ((void)0)
#define RB_SPAN_END(slot) ((void)0)
#define RB_WGT_ROLE(kid, wg, role) ((void)0)
#define RB_CSTAMP(i) ((void)0)
#define RB_CSTAMP_LAST(i) ((void)0)
#define RB_FSTAMP(on, i) ((void)0)
#define RB_WGT(kid, wg, slot) ((void)0)
#define RB_WGT_HW(kid, wg) ((void)0)
#endif
