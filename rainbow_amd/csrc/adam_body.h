// adam_body.h — clip_grad_norm_ + Adam (agent.py:97-98) as a device body that a foreign launch can host.
// k_clip_adam (adam_kernels.h) runs it as a launch of its own; k_sample (replay_sample.h) can carry it as extra workgroups: the
// optimiser pass of learn call k has no data dependency on the sampler of call k + 1 (it reads the gradient, its norm
// partials and the moments; the sampler reads the sum-tree, whose write-back happened in call k's backward), so when two
// learn calls follow each other the 6.4 M-parameter streaming pass runs beside the sampler's serial, latency-bound
// workgroup instead of in front of it.  Same arithmetic, same summation order: the parameters are bit-identical.
#pragma once
#include "rb_common.h"

// clip_grad_norm_ + Adam in ONE pass over the flat buffers (agent.py:97-98).  Every block re-sums the partial list in the
// same fixed order (so all blocks agree on the clip coefficient) while its first parameter/gradient/moment loads are
// already in flight, then applies torch.optim.Adam's single-tensor update:
//   g' = g * clamp(max_norm / (norm + 1e-6), max=1)                       (clip_grad_norm_)
//   m  = lerp(m, g', 1-b1);  v = v*b2 + (1-b2)*g'*g'
//   p += -(lr / (1-b1^t)) * m / (sqrt(v) / sqrt(1-b2^t) + eps)
// The scaled gradient is stored back only when the clip actually bites (the reference leaves .grad scaled).
struct ClipAdamArgs {
  float* p; float* g; float* m; float* v;
  int64_t n;
  const float* part; int nparts;
  float max_norm; float* norm_out;
  float w1, b2, w2, neg_step_size, bc2_sqrt, eps;
  // hipGraph replay / hosted pass: the step number lives on the device (rb_learner_set_step_counter; incremented by the
  // head kernel of every learn call), and the bias corrections 1 - beta^t are formed here, in double like the host path,
  // by one thread per block — by-value scalars would freeze at capture time
  const long long* step_dev;
  double lr, beta1, beta2;
  // FUSED: elements [skip_lo, skip_lo + skip_len) (the hidden layer's mu | sigma weight arrays) are not touched by the
  // elementwise part: the tile part updates them from gradients it recomputes on the fly
  int64_t skip_lo4, skip_len4;        // in float4 units
  // non-NULL and non-zero on the device: the batch behind this gradient was not a legal one (the sampler gave up; its
  // importance weights are zero and so is the gradient) — the whole update is skipped instead of letting Adam's momentum
  // move the parameters on a step the reference would never have taken
  const int32_t* batch_status;
  // IMPLICIT sigma gradient (RB_LEARNER_IMPLICIT_SIGMA, hosted pass only): the hidden layer's sigma-weight gradient is
  // g_mu * (eps_out[n] * eps_in[k]) element for element (model.py:44's product rule; the backward forms exactly this), so the
  // backward does not store it and this pass does not load it: quads [pair_mu4, pair_mu4 + pair_len4) (mu) and the pair_len4
  // quads behind them (sigma) are updated TOGETHER by the pair workgroups [pair_blk0, nblk) — 7 loads instead of 8, and
  // 12.85 MB less written by the backward at the canonical shape.  eps come from a snapshot the backward took (the launch that
  // hosts this pass also resamples the noise).  The scaled gradients are stored back when the clip bites, sigma's included.
  int64_t pair_mu4, pair_len4;
  unsigned hole_lo4, hole4;    // the same range for the plain workgroups, which walk the quads OUTSIDE it: virtual quad j is quad j
                               // below hole_lo4 and quad j + hole4 from there on (hole4 = 0: no pairing)
  int pair_blk0;               // first pair workgroup (= number of plain workgroups)
  int pair_f4, pair_split_row; // quads per weight row; rows >= split_row take eps_in from the second stream's vector
  float tau;                   // (in what was padding) target EMA, see `t` below: 0 = off, 1 = the target copies p
  const float* pair_eout;      // [rows]
  const float* pair_ein;       // [2][4 * pair_f4]
  int32_t* pair_clipped;       // written by the pair pass: 1 = the clip bit and the SCALED gradients (sigma's included) were stored
                               // back, exactly as the reference leaves .grad — a later materialisation must not redo them from
                               // the scaled g_mu (the product would round in another order); 0 = nothing was stored
  // TARGET EMA (rb_learner_set_target_tau; the EMA instantiations of the kernels only): non-NULL = the target network's flat
  // parameters follow the update in the same pass, t += tau (p_new - t) element for element (rb_ema_elem) — the new p is in a
  // register here, a pass of its own would read it back.  A skipped update (batch_status) leaves t alone as it leaves p.
  float* t;
};
static_assert(sizeof(ClipAdamArgs) <= 256, "ClipAdamArgs: the device copy (adam_args_dev, rb_debug_adam_pass) is 256 bytes");
// (IEEE sqrt and divisions, as torch computes them: hardware rcp / approximate sqrt measured 1.5 us faster per launch
// and stay far inside the test tolerance, but the update would no longer be the reference's formula rounding for rounding)
__device__ __forceinline__ void rb_adam_elem(float& p, float& g, float& m, float& v, float coef, const ClipAdamArgs& a) {
  g = g * coef;
  m = fmaf(a.w1, g - m, m);
  v = v * a.b2 + a.w2 * g * g;
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  p = p + a.neg_step_size * (m / denom);
}
__device__ __forceinline__ void rb_adam_quad(float4& P, float4& G, float4& M, float4& V, float coef, const ClipAdamArgs& a) {
  rb_adam_elem(P.x, G.x, M.x, V.x, coef, a);
  rb_adam_elem(P.y, G.y, M.y, V.y, coef, a);
  rb_adam_elem(P.z, G.z, M.z, V.z, coef, a);
  rb_adam_elem(P.w, G.w, M.w, V.w, coef, a);
}

// The target network's EMA step on the freshly written parameter: t <- t + tau (p - t), one rounding for the difference and one
// for the fma (written out like m's: the unit is built with -ffp-contract=off).  tau == 1 is a case of its own for the
// callers (rb_ema_quad: t = p, and t is never loaded): fmaf(1, p - t, t) is not p bit for bit.
__device__ __forceinline__ void rb_ema_elem(float& t, float p, float tau) {
  t = fmaf(tau, p - t, t);
}
// copy = (tau == 1), wave-uniform
__device__ __forceinline__ void rb_ema_quad(float4& T, const float4& P, float tau, bool copy) {
  if (copy) { T = P; return; }
  rb_ema_elem(T.x, P.x, tau); rb_ema_elem(T.y, P.y, tau); rb_ema_elem(T.z, P.z, tau); rb_ema_elem(T.w, P.w, tau);
}

// The plain pass (no skipped range) as hosted workgroups: block `eb` of `nblk`.  The element loops work for any block size that
// is a multiple of 64, but the prologue hands norm partial i to thread i % blockDim.x, so the summation order — and with it the
// bit-identity with k_clip_adam (adam_kernels.h), which is always 256 threads — holds at 256 threads only; every caller launches
// 256 (replay.hip sample_impl, k_adam_pending).
// The arguments live in DEVICE memory (`ad`; the host rewrites them only when a pointer or a hyper-parameter changes, with
// k_store_adam_args in a launch of its own): by value they would occupy ~50 SGPRs of the hosting kernel on every path.  They are
// read through the SCALAR path (rb_ld_uniform), so every field is wave-uniform to the compiler: fetched with vector loads the
// pointers sat in VGPRs, every buffer descriptor was "divergent", and each load and store of the pass was wrapped in a
// waterfall loop (4 v_readfirstlane, two compares, s_and_saveexec, the access, a branch: 350 readfirstlanes and 91 loops in
// the hosted region of the sampler kernel, profiles/hosted_pass_isa.txt).  Pointers that come out of memory are generic
// pointers — every access goes through a buffer descriptor instead (no flat instructions; 32-bit byte offsets: the caller
// guarantees 4 n < 2^31).  Requires a.step_dev (the step number cannot be a launch-time scalar here).
//
// ONE memory trip per workgroup.  Everything a workgroup reads is requested before its first wait, earliest-consumed first
// (vmcnt retires in order): the batch status, the step number, the thread's first 16 norm partials (rb_adam_hosted_request),
// the pair workgroups' noise factors, then the p / g / m / v quads.  The status branch, the partial sum, rb_block_sum's two
// barriers and the bias corrections then run while the quads are in flight (before, the status word was loaded BEHIND the
// quads and its wait drained them, and only then were the partials requested: three dependent trips per pair workgroup).
struct rb_adam_req {
  float status;                // raw bits of *batch_status (0 without one)
  unsigned st_lo, st_hi;       // the step number's halves
  float pv[16];                // partials threadIdx.x + u * blockDim.x (clamped to the last one)
};
__device__ __forceinline__ void rb_adam_hosted_request(const ClipAdamArgs& a, rb_adam_req& q) {
  const unsigned T = blockDim.x;
  q.status = 0.0f;
  if (a.batch_status) q.status = rb_ld1_buf(rb_make_buf(a.batch_status), 0, 0);     // (uniform branch; every lane, one address)
  const rb_buf bs = rb_make_buf(a.step_dev);                                        // (every lane: no divergent branch between the loads)
  q.st_lo = __builtin_bit_cast(unsigned, rb_ld1_buf(bs, 0, 0)); q.st_hi = __builtin_bit_cast(unsigned, rb_ld1_buf(bs, 4, 0));
  const rb_buf bpart = rb_make_buf(a.part);
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int i = (int)threadIdx.x + u * (int)T;
    q.pv[u] = rb_ld1_buf(bpart, 4u * (unsigned)(i < a.nparts ? i : a.nparts - 1), 0);
  }
}
// everything between a hosted workgroup's loads and its update: batch status, the norm from the partial list (fixed order:
// thread t adds partials t, t + T, t + 2 T, ... in index order, then rb_block_sum), the bias corrections from the device step
// counter.  Returns false when the update is to be skipped.
__device__ __forceinline__ bool rb_adam_hosted_prologue(ClipAdamArgs& a, int eb, const rb_adam_req& q, float* s_red16, float* coef_out) {
  const unsigned T = blockDim.x;
  float acc = 0.0f;
#pragma unroll
  for (int u = 0; u < 16; ++u)
    if ((int)threadIdx.x + u * (int)T < a.nparts) acc += q.pv[u];
  {
    // lists beyond 16 T partials: 16 in flight per further trip (a loop of single loads is one L2 round trip per iteration)
    const rb_buf bpart = rb_make_buf(a.part);
    for (int i0 = (int)threadIdx.x + 16 * (int)T; i0 < a.nparts; i0 += 16 * (int)T) {
      float pv[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = i0 + u * (int)T;
        pv[u] = rb_ld1_buf(bpart, 4u * (unsigned)(i < a.nparts ? i : a.nparts - 1), 0);
      }
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (i0 + u * (int)T < a.nparts) acc += pv[u];
    }
  }
  if (threadIdx.x == 0) {
    const double t = (double)(long long)(((unsigned long long)q.st_hi << 32) | q.st_lo);
    const double bc1 = 1.0 - pow(a.beta1, t), bc2 = 1.0 - pow(a.beta2, t);
    s_red16[16] = (float)(-(a.lr / bc1));
    s_red16[17] = (float)sqrt(bc2);
  }
  acc = rb_block_sum(acc, s_red16);
  // the status branch BEHIND the sum (a skipped update is the rare case and may pay for a sum it drops): in front of it the
  // compiler sank the partial loads into the branch's far side, behind the status word's round trip
  if (rb_wave_uniform(__builtin_bit_cast(int, q.status)) != 0) {   // block-uniform
    if (eb == 0 && threadIdx.x == 0 && a.norm_out) rb_st1_wt(a.norm_out, 0, 0.0f);
    return false;
  }
  const float total = sqrtf(acc);
  float coef = a.max_norm / (total + 1e-6f);
  if (coef > 1.0f) coef = 1.0f;                                    // clamp(max=1.0)
  if (eb == 0 && threadIdx.x == 0 && a.norm_out) rb_st1_wt(a.norm_out, 0, total);
  a.neg_step_size = s_red16[16];                                   // (written before rb_block_sum's barriers)
  a.bc2_sqrt = s_red16[17];
  *coef_out = coef;
  return true;
}

// pair workgroup `pb` (0-based among the pair workgroups): 2 (mu, sigma) quad pairs per thread = 14 data quads in flight, behind
// the prologue's requests and the noise factors eps_out / eps_in of the thread's pairs (10 registers; their products are formed
// when the update needs them.  With one pair per thread the pass streamed too thinly to gain anything: 38.8 against 36.3 us
// for the hosting launch).
// EMA: the target's (mu, sigma) quads join the same trip (requested last: consumed last; not at all when tau == 1) and are
// written with the same write-through stores.
template <bool EMA>
__device__ __forceinline__ void rb_adam_hosted_pairs(ClipAdamArgs& a, int eb, int pb, float* s_red16) {
  constexpr int PU = 2;
  const unsigned T = blockDim.x;
  const unsigned len4 = (unsigned)a.pair_len4, mu4 = (unsigned)a.pair_mu4;
  const unsigned base = (unsigned)pb * (T * PU) + threadIdx.x;
  rb_adam_req q;
  rb_adam_hosted_request(a, q);
  const rb_buf beo = rb_make_buf(a.pair_eout), bei = rb_make_buf(a.pair_ein);
  float4 E[PU];
  float eo[PU];
#pragma unroll
  for (int u = 0; u < PU; ++u) {
    unsigned j = base + u * T;
    if (j >= len4) j = len4 - 1;
    const unsigned row = j / (unsigned)a.pair_f4, cq = j - row * (unsigned)a.pair_f4;
    eo[u] = rb_ld1_buf(beo, 4 * row, 0);
    E[u] = rb_ld4_buf(bei, 16 * (cq + ((int)row >= a.pair_split_row ? (unsigned)a.pair_f4 : 0u)), 0);
  }
  const rb_buf bp = rb_make_buf(a.p), bg = rb_make_buf(a.g), bm = rb_make_buf(a.m), bv = rb_make_buf(a.v);
  float4 P[PU], G[PU], M[PU], V[PU], P2[PU], M2[PU], V2[PU];
#pragma unroll
  for (int u = 0; u < PU; ++u) {
    unsigned j = base + u * T;
    if (j >= len4) j = len4 - 1;                         // clamped loads (always legal), masked stores
    const unsigned i = mu4 + j, i2 = i + len4;
    P[u] = rb_ld4_buf(bp, 16 * i, 0); G[u] = rb_ld4_buf(bg, 16 * i, 0);
    M[u] = rb_ld4_buf(bm, 16 * i, 0); V[u] = rb_ld4_buf(bv, 16 * i, 0);
    P2[u] = rb_ld4_buf(bp, 16 * i2, 0); M2[u] = rb_ld4_buf(bm, 16 * i2, 0); V2[u] = rb_ld4_buf(bv, 16 * i2, 0);
  }
  const bool ema_copy = EMA && a.tau == 1.0f;            // uniform
  float4 TG[EMA ? PU : 1], TG2[EMA ? PU : 1];
  if (EMA && !ema_copy) {
    const rb_buf bt = rb_make_buf(a.t);
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      unsigned j = base + u * T;
      if (j >= len4) j = len4 - 1;
      TG[u] = rb_ld4_buf(bt, 16 * (mu4 + j), 0); TG2[u] = rb_ld4_buf(bt, 16 * (mu4 + j + len4), 0);
    }
  }
  float coef;
  if (!rb_adam_hosted_prologue(a, eb, q, s_red16, &coef)) return;
  if (pb == 0 && threadIdx.x == 0 && a.pair_clipped) rb_st1_wt(reinterpret_cast<float*>(a.pair_clipped), 0, __builtin_bit_cast(float, coef < 1.0f ? 1 : 0));
#pragma unroll
  for (int u = 0; u < PU; ++u) {
    const unsigned j = base + u * T;
    if (j >= len4) continue;
    const unsigned i = mu4 + j, i2 = i + len4;
    float4 pr;                                           // eps_out * eps_in: the inner product of the backward's g_mu * (eo * e)
    pr.x = eo[u] * E[u].x; pr.y = eo[u] * E[u].y; pr.z = eo[u] * E[u].z; pr.w = eo[u] * E[u].w;
    float4 G2;                                           // the backward's own expression: g_sigma = g_mu * (eps_out * eps_in)
    G2.x = G[u].x * pr.x; G2.y = G[u].y * pr.y; G2.z = G[u].z * pr.z; G2.w = G[u].w * pr.w;
    rb_adam_quad(P[u], G[u], M[u], V[u], coef, a);
    rb_adam_quad(P2[u], G2, M2[u], V2[u], coef, a);
    rb_st4_wt(a.p, 16 * i, P[u]); rb_st4_wt(a.m, 16 * i, M[u]); rb_st4_wt(a.v, 16 * i, V[u]);
    rb_st4_wt(a.p, 16 * i2, P2[u]); rb_st4_wt(a.m, 16 * i2, M2[u]); rb_st4_wt(a.v, 16 * i2, V2[u]);
    if (coef < 1.0f) { rb_st4_wt(a.g, 16 * i, G[u]); rb_st4_wt(a.g, 16 * i2, G2); }
    if (EMA) {
      rb_ema_quad(TG[u], P[u], a.tau, ema_copy); rb_ema_quad(TG2[u], P2[u], a.tau, ema_copy);
      rb_st4_wt(a.t, 16 * i, TG[u]); rb_st4_wt(a.t, 16 * i2, TG2[u]);
    }
  }
}

template <int UNROLL, bool EMA = false>
__device__ __forceinline__ void rb_adam_hosted_block(const ClipAdamArgs* ad, int eb, int nblk, float* s_red16 /* [18] */) {
  ClipAdamArgs a = rb_ld_uniform(ad);                    // SGPRs; each role keeps only the fields it uses
  const int nplain = a.hole4 > 0 ? a.pair_blk0 : nblk;
  if (eb >= nplain) {                                    // block-uniform: a (mu, sigma) pair workgroup
    rb_adam_hosted_pairs<EMA>(a, eb, eb - nplain, s_red16);
    return;
  }
  const unsigned T = blockDim.x;
  const unsigned n4 = (unsigned)(a.n >> 2);
  const unsigned hole_lo = a.hole4 > 0 ? a.hole_lo4 : n4, hole = a.hole4;
  const unsigned nv4 = n4 - hole;
  auto real_of = [&](unsigned j) { return j < hole_lo ? j : j + hole; };
  const unsigned base = (unsigned)eb * (T * UNROLL) + threadIdx.x;
  const rb_buf bp = rb_make_buf(a.p), bg = rb_make_buf(a.g), bm = rb_make_buf(a.m), bv = rb_make_buf(a.v);
  rb_adam_req q;
  rb_adam_hosted_request(a, q);
  float4 P[UNROLL], G[UNROLL], M[UNROLL], V[UNROLL];
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    unsigned j = base + u * T;
    if (j >= nv4) j = nv4 > 0 ? nv4 - 1 : 0;         // clamped load (always legal), masked store
    const unsigned i = real_of(j);
    P[u] = rb_ld4_buf(bp, 16 * i, 0); G[u] = rb_ld4_buf(bg, 16 * i, 0);
    M[u] = rb_ld4_buf(bm, 16 * i, 0); V[u] = rb_ld4_buf(bv, 16 * i, 0);
  }
  // EMA: the target's quads (and its tail element) behind them in the same trip — consumed last; none when tau == 1
  const bool ema_copy = EMA && a.tau == 1.0f;            // uniform
  const bool has_tail = eb == nplain - 1 && ((a.n >> 2) << 2) + threadIdx.x < a.n;
  const unsigned tail_off = (unsigned)(4 * (((a.n >> 2) << 2) + threadIdx.x));
  float4 TG[EMA ? UNROLL : 1];
  float tg_tail = 0.0f;
  if (EMA && !ema_copy) {
    const rb_buf bt = rb_make_buf(a.t);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      unsigned j = base + u * T;
      if (j >= nv4) j = nv4 > 0 ? nv4 - 1 : 0;
      TG[u] = rb_ld4_buf(bt, 16 * real_of(j), 0);
    }
    if (has_tail) tg_tail = rb_ld1_buf(bt, tail_off, 0);
  }
  float coef;
  if (!rb_adam_hosted_prologue(a, eb, q, s_red16, &coef)) return;
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const unsigned j = base + u * T;
    if (j >= nv4) continue;
    const unsigned i = real_of(j);
    rb_adam_quad(P[u], G[u], M[u], V[u], coef, a);
    rb_st4_wt(a.p, 16 * i, P[u]); rb_st4_wt(a.m, 16 * i, M[u]); rb_st4_wt(a.v, 16 * i, V[u]);
    if (coef < 1.0f) rb_st4_wt(a.g, 16 * i, G[u]);
    if (EMA) {
      rb_ema_quad(TG[u], P[u], a.tau, ema_copy);
      rb_st4_wt(a.t, 16 * i, TG[u]);
    }
  }
  // tail (n % 4 elements): the last plain block's first threads
  if (eb == nplain - 1) {
    const int64_t t = ((a.n >> 2) << 2) + threadIdx.x;
    if (t < a.n) {
      const unsigned o = (unsigned)(4 * t);
      float p = rb_ld1_buf(bp, o, 0), g = rb_ld1_buf(bg, o, 0), m = rb_ld1_buf(bm, o, 0), v = rb_ld1_buf(bv, o, 0);
      rb_adam_elem(p, g, m, v, coef, a);
      rb_st1_wt(a.p, o, p); rb_st1_wt(a.m, o, m); rb_st1_wt(a.v, o, v);
      if (coef < 1.0f) rb_st1_wt(a.g, o, g);
      if (EMA) {
        if (ema_copy) tg_tail = p; else rb_ema_elem(tg_tail, p, a.tau);
        rb_st1_wt(a.t, o, tg_tail);
      }
    }
  }
}

// The pending pass as a launch of its own through the HOSTED body (adam_kernels.h k_adam_pending, in the learner's unit; arguments
// in device memory): what runs a pass with (mu, sigma) pairing outside a sampler launch.  Returns RB_OK or RB_ERR_HIP.
// ema: the pass's arguments carry a target (k_adam_pending_ema; the caller knows: the arguments live on the device).
int rb_launch_adam_pending(const ClipAdamArgs* args_dev, int blocks, void* stream, bool ema = false);
