// param_reset.h — shrink-and-perturb parameter resets (Ash & Adams 2020; the periodic resets of SR-SPR / BBF):
//     theta <- alpha * theta + (1 - alpha) * phi      per named tensor, phi a FRESH draw from the tensor's initial distribution
// as ONE launch over the flat buffers: online parameters, target parameters (the same phi) and both Adam moments (cleared where
// alpha < 1).  Included by learner.hip only, after optimizer_host.h (flush_update).  Never on the per-step path: a run that does
// not reset launches exactly what it launched before this file existed.
//
// The draw of flat element i depends on (seed, draw, i) alone, never on the grid or on the tensor order: word i & 3 of
// rb_philox(seed ^ RB_RESET_KEY_TAG, draw, i >> 2);  u = (float)(x >> 8) * 2^-24,  r = 2u - 1,  phi = bound * r  (bound rounded to
// f32 by the host).  Tensors whose initial value is a constant (the sigma tensors) take that constant as phi.
//     new = alpha * theta + om * phi      two products, one sum, no FMA (-ffp-contract=off), om = 1.0f - alpha formed by the host
// alpha == 0 writes phi without reading theta (a non-finite theta does not survive a full reset; online and target come out
// bit-equal: the tau == 1 path of the EMA has the same shape); tensors with alpha == 1 are not in the table at all: neither read
// nor written, like the align64 padding between the tensors, which belongs to no descriptor.
#pragma once
#include "learner_internal.h"

#define RB_RESET_KEY_TAG 0x5245534554ull      // "RESET": a key of its own (the shift gather's is RB_SHIFT_KEY_TAG, replay_shift.h)
#define RB_RESET_MAX_DESC 22                  // 2 * nconv + 16 named tensors (layout_api.h rb_learner_param_layout)

struct ResetDesc {
  int32_t off, count;     // the tensor's floats [off, off + count) of the flat buffer
  float val;              // uniform != 0: the bound of U(-bound, bound); else the constant
  float alpha, om;        // om = 1.0f - alpha
  int32_t uniform;
};
// By value in the kernel's argument block: every field is read through the scalar path, the loop over the table is wave-uniform
struct ResetTable {
  int32_t n, pad_;
  ResetDesc d[RB_RESET_MAX_DESC];
};

__device__ __forceinline__ float rb_reset_mix(float alpha, float om, float phi, float theta) {
  return alpha == 0.0f ? phi : alpha * theta + om * phi;
}

extern "C" {

// One workgroup = 1024 flat-aligned quads, thread t takes quads t, t + 256, t + 512, t + 768 of them: one Philox call per quad,
// 16-byte accesses, the four quads' loads of theta and of the target issued before the first use (32 KiB in flight per workgroup).
// Tensor offsets are no multiples of 4 (fc_z_a.bias_* starts `atoms` floats into its segment), so the tensor of an element is
// looked up per ELEMENT — a wave-uniform walk over the descriptors that meet this workgroup's range, nearly always one — and a
// quad that is not covered whole (a tensor's edge against padding or against an alpha == 1 tensor) goes element by element.
// t, m, v may be NULL (no target / no moments to touch); the caller launches nothing when the table is empty.
__global__ __launch_bounds__(256) void k_shrink_perturb(ResetTable tab, float* p, float* t, float* m, float* v, uint64_t key, uint64_t draw) {
  const int tid = (int)threadIdx.x;
  const int blk_lo = (int)blockIdx.x * 4096;                   // (the host has checked that the buffer's indices fit 31 bits)
  float al[4][4], om[4][4], val[4][4];
  unsigned hit = 0u, uni = 0u;                                 // bit 4 * u + e: element e of quad u belongs to a descriptor / is drawn
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) { al[u][e] = 1.0f; om[u][e] = 0.0f; val[u][e] = 0.0f; }
  for (int d = 0; d < tab.n; ++d) {
    const int off = tab.d[d].off, cnt = tab.d[d].count;
    if (off + cnt <= blk_lo || off >= blk_lo + 4096) continue;  // block-uniform
    const float da = tab.d[d].alpha, dom = tab.d[d].om, dval = tab.d[d].val;
    const unsigned duni = tab.d[d].uniform ? 1u : 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int idx = blk_lo + 4 * (u * 256 + tid) + e;
        if ((unsigned)(idx - off) < (unsigned)cnt) {
          al[u][e] = da; om[u][e] = dom; val[u][e] = dval;
          hit |= 1u << (4 * u + e);
          uni |= duni << (4 * u + e);
        }
      }
  }
  float4 P[4], T[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t q = (int64_t)blockIdx.x * 1024 + u * 256 + tid;
    P[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); T[u] = P[u];
    const bool whole = ((hit >> (4 * u)) & 15u) == 15u;
    const bool reads = al[u][0] != 0.0f || al[u][1] != 0.0f || al[u][2] != 0.0f || al[u][3] != 0.0f;
    if (whole && reads) {
      P[u] = rb_ld4(p + 4 * q);
      if (t) T[u] = rb_ld4(t + 4 * q);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const unsigned mk = (hit >> (4 * u)) & 15u;
    if (mk == 0u) continue;
    const int64_t q = (int64_t)blockIdx.x * 1024 + u * 256 + tid;
    float phi[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) phi[e] = val[u][e];
    if ((uni >> (4 * u)) & 15u) {
      const rb_philox_out r = rb_philox(key, draw, (uint64_t)q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float un = (float)(r.v[e] >> 8) * 0x1p-24f;
        const float sym = 2.0f * un - 1.0f;
        if ((uni >> (4 * u + e)) & 1u) phi[e] = val[u][e] * sym;
      }
    }
    if (mk == 15u) {
      float4 o;
      o.x = rb_reset_mix(al[u][0], om[u][0], phi[0], P[u].x); o.y = rb_reset_mix(al[u][1], om[u][1], phi[1], P[u].y);
      o.z = rb_reset_mix(al[u][2], om[u][2], phi[2], P[u].z); o.w = rb_reset_mix(al[u][3], om[u][3], phi[3], P[u].w);
      rb_st4(p + 4 * q, o);
      if (t) {
        o.x = rb_reset_mix(al[u][0], om[u][0], phi[0], T[u].x); o.y = rb_reset_mix(al[u][1], om[u][1], phi[1], T[u].y);
        o.z = rb_reset_mix(al[u][2], om[u][2], phi[2], T[u].z); o.w = rb_reset_mix(al[u][3], om[u][3], phi[3], T[u].w);
        rb_st4(t + 4 * q, o);
      }
      const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (m) rb_st4(m + 4 * q, z);
      if (v) rb_st4(v + 4 * q, z);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (!((mk >> e) & 1u)) continue;
        const int64_t i = 4 * q + e;
        const float a = al[u][e];
        p[i] = rb_reset_mix(a, om[u][e], phi[e], a == 0.0f ? 0.0f : p[i]);
        if (t) t[i] = rb_reset_mix(a, om[u][e], phi[e], a == 0.0f ? 0.0f : t[i]);
        if (m) m[i] = 0.0f;
        if (v) v[i] = 0.0f;
      }
    }
  }
}

}  // extern "C"

static void reset_add(ResetTable* T, int64_t off, int64_t count, bool uniform, float val, float alpha) {
  if (!(alpha < 1.0f) || count <= 0) return;       // alpha == 1: the tensor and its moments stay untouched, unread and unwritten
  ResetDesc& d = T->d[T->n++];
  d.off = (int32_t)off; d.count = (int32_t)count; d.val = val; d.alpha = alpha; d.om = 1.0f - alpha; d.uniform = uniform ? 1 : 0;
}

// The distributions of agent.py init_parameters_flat (model.py:25-30 and torch.nn.Conv2d.reset_parameters) over the named tensors
// of rb_learner_param_layout, in its order.  Bounds and constants are formed in double and rounded once to f32.
static void reset_table(const Layout& L, float alpha_encoder, float alpha_head, float noisy_std, ResetTable* T) {
  memset(T, 0, sizeof(*T));
  for (int l = 0; l < L.nconv; ++l) {
    const ConvLayer& c = L.conv[l];
    const float bound = (float)(1.0 / sqrt((double)c.K()));                      // U(+-1/sqrt(fan_in)), weight and bias
    reset_add(T, L.conv_w[l], (int64_t)c.cout * c.K(), true, bound, alpha_encoder);
    reset_add(T, L.conv_b[l], c.cout, true, bound, alpha_encoder);
  }
  const double std = (double)noisy_std;
  const int64_t HF = (int64_t)L.H * L.F, ZH = (int64_t)L.Z * L.H;
  const float bF = (float)(1.0 / sqrt((double)L.F)), bH = (float)(1.0 / sqrt((double)L.H));
  const float sF = (float)(std / sqrt((double)L.F)), sH = (float)(std / sqrt((double)L.H));
  for (int s = 0; s < 2; ++s) {                                                  // fc_h_v, fc_h_a: in = F, out = H
    reset_add(T, L.h_mu + s * HF, HF, true, bF, alpha_head);
    reset_add(T, L.h_sigma + s * HF, HF, false, sF, alpha_head);
    reset_add(T, L.h_bmu + s * L.H, L.H, true, bF, alpha_head);
    reset_add(T, L.h_bsigma + s * L.H, L.H, false, sH, alpha_head);
  }
  for (int s = 0; s < 2; ++s) {                                                  // fc_z_v: in = H, out = Z; fc_z_a: out = A * Z
    const int64_t rows = s == 0 ? L.Z : (int64_t)L.A * L.Z, row0 = s == 0 ? 0 : L.Z;
    reset_add(T, L.z_mu + s * ZH, rows * L.H, true, bH, alpha_head);
    reset_add(T, L.z_sigma + s * ZH, rows * L.H, false, sH, alpha_head);
    reset_add(T, L.z_bmu + row0, rows, true, bH, alpha_head);
    reset_add(T, L.z_bsigma + row0, rows, false, (float)(std / sqrt((double)rows)), alpha_head);
  }
}

extern "C" {

int rb_learner_shrink_perturb(rb_learner_t* l, float alpha_encoder, float alpha_head, float noisy_std, uint64_t seed, uint64_t draw,
                              int32_t with_target, float* exp_avg_dev, float* exp_avg_sq_dev, rb_stream_t stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_shrink_perturb: NULL handle");
  RB_REQUIRE(alpha_encoder >= 0.0f && alpha_encoder <= 1.0f, "rb_learner_shrink_perturb: alpha_encoder must be in [0, 1], got %g",
             (double)alpha_encoder);
  RB_REQUIRE(alpha_head >= 0.0f && alpha_head <= 1.0f, "rb_learner_shrink_perturb: alpha_head must be in [0, 1], got %g", (double)alpha_head);
  RB_REQUIRE(noisy_std >= 0.0f && noisy_std < INFINITY, "rb_learner_shrink_perturb: noisy_std must be finite and >= 0, got %g",
             (double)noisy_std);
  RB_REQUIRE((exp_avg_dev == nullptr) == (exp_avg_sq_dev == nullptr), "rb_learner_shrink_perturb: pass both moment buffers or neither");
  RB_REQUIRE(((uintptr_t)exp_avg_dev | (uintptr_t)exp_avg_sq_dev) % 16 == 0, "rb_learner_shrink_perturb: the moment buffers must be 16-byte aligned");
  const int64_t n = l->L.n_params;
  RB_REQUIRE(n * 4 < (int64_t)0x7fffffff, "rb_learner_shrink_perturb: the flat parameter buffer must be smaller than 2 GiB");
  static_assert(sizeof(ResetTable) == 8 + 24 * RB_RESET_MAX_DESC, "ResetTable: whole words, no holes");
  RB_FLUSH_UPDATE(l, stream);          // a pending pass belongs to the OLD tensors: it runs before the reset, never after it
  ResetTable tab;
  reset_table(l->L, alpha_encoder, alpha_head, noisy_std, &tab);
  if (tab.n == 0) return RB_OK;        // alpha == 1 everywhere: nothing changes
  RB_LAUNCH(k_shrink_perturb, dim3((unsigned)rb_div_up(n, 4096)), dim3(256), stream, tab, l->p_online, with_target ? l->p_target : (float*)nullptr,
            exp_avg_dev, exp_avg_sq_dev, seed ^ RB_RESET_KEY_TAG, draw);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

}  // extern "C"
