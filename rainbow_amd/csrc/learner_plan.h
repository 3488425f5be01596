// learner_plan.h — WHICH kernel a shape reaches, and with what grid: every such decision of the learner, as pure functions from
// (Layout, RbOpts, LearnerCaps, compute units, flags, exchange / sink state, this call's row counts) to plain structs.  No launches,
// no device memory.  The launch functions (conv_dispatch.h, fc_dispatch.h, learner.hip) take a plan, fill the argument struct and
// switch on the kernel id; rb_debug_launch_plan (launch_plan_debug.h) prints the same plans, and tests/test_launch_plan.py pins them
// against DESIGN.md §3 / §8.  Plans are computed per call, where the decisions were always taken: nothing here is cached.
#pragma once
#include "learner_internal.h"

// floats of rb_learner::norm_part: the sum-of-squares partials one step may leave for the clip (plan_fc_bwd fuse_norm, exchange_host.h plan_finish)
#define RB_NORM_PART_SLOTS 16384

struct PlanIn {
  const Layout& L;
  const RbOpts& opt;
  const LearnerCaps& caps;
  int n_cu, flags;
  bool exch;      // replica exchange active (world > 1 with its buffers set, streamed FC kernels): FC weight gradients are deferred
  bool sink;      // a priority sink is set: the learn step writes loss^w back into the replay's sum-tree itself
};

static int pick_splits(int64_t tiles, int ksteps, int64_t target_blocks) {
  int64_t s = target_blocks / (tiles > 0 ? tiles : 1);
  if (s < 1) s = 1;
  if (s > ksteps) s = ksteps;
  if (s > 64) s = 64;
  const int64_t per = (ksteps + s - 1) / s;   // no empty trailing split (every partial slice gets written)
  s = (ksteps + per - 1) / per;
  return (int)s;
}

// ------------------------------------------------------------------------- caps --
static LearnerCaps plan_caps(const Layout& L, const RbOpts& opt) {
  LearnerCaps c;
  memset(&c, 0, sizeof(c));
  const int B = L.B;
  const int generic = opt.generic;
  c.fast_fc = (L.F % 32 == 0 && L.H % 32 == 0 && L.F <= RB_NL_FWD_KMAX && L.H <= RB_NL_FWD_KMAX && generic == 0) ? 1 : 0;
  c.fast_conv = (L.hist <= 4 && generic != 1) ? 1 : 0;
  // split-K factors: aim for >= ~2 workgroups per CU on the 256-CU part
  if (c.fast_fc) {
    c.hs = pick_splits(2 * rb_div_up(L.H, 32) * 2 * rb_div_up(2 * B, 64), L.F / 16 / RB_NL_FWD_WAVES, 512);
    // input-gradient row splits: 256 weight rows per workgroup (64 per wave = 4 sixteen-row iterations); measured
    // 225.1 us per step against 228.3 with the former ~100-row splits (xs 10) and 239 without splitting
    // (at most 4: the consumers of the partials — the last conv layer's dX and dW kernels — sum up to 4 of them while staging)
    c.xs = (int)rb_div_up(2 * L.H, 256);
    if (c.xs > 4) c.xs = 4;
    if (opt.xs > 0) c.xs = opt.xs;
  } else {
    c.hs = pick_splits(rb_div_up(2 * B, 64) * rb_div_up(2 * L.H, 64) * 2, (L.F + 15) / 16, 512);
    c.xs = pick_splits(rb_div_up(B, 32) * rb_div_up(L.F, 64), (2 * L.H + 15) / 16, 512);
  }
  for (int i = 0; i < L.nconv; ++i) {
    const ConvLayer& cl = L.conv[i];
    const int64_t tiles = i == 0 ? rb_div_up(cl.cout, 32) * rb_div_up(cl.K() + 1, 64)
                                 : rb_div_up(cl.cout, 64) * rb_div_up(cl.K() + 1, 64);
    c.ws[i] = pick_splits(tiles, (B * cl.P() + 15) / 16, 512);
    c.wT[i] = (i > 0 && c.fast_conv && cl.cin % 32 == 0) ? 1 : 0;
  }
  c.gemm_ws = (c.fast_fc && opt.fc_gemm != 0) ? 1 : 0;
  return c;
}

// --------------------------------------------------------------------- geometry --
// The five conv geometries with the tile parameters of their forward kernels (conv_fwd.h): NT 32-position tiles per workgroup,
// PR patch rows, KMAX reduction length staged, FIRST = reads frames, PCH output positions per workgroup.
template <class G_, int NT_, int PR_, int KMAX_, bool FIRST_, int PCH_ = 32 * NT_>
struct ConvCfg {
  using G = G_;
  static constexpr int NT = NT_, PR = PR_, KMAX = KMAX_, PCH = PCH_;
  static constexpr bool FIRST = FIRST_;
  // whole-K 16x16x4 tiles, one wave per tile, no cross-wave reduction (conv_fwd_image.h T16).  Every later layer of the canonical stack
  // qualifies (cin * KK == KMAX and cout % 32 == 0 by construction); the data-efficient ones do not (K % 16 != 0, 9 positions)
  static constexpr bool T16_OK = KMAX % 16 == 0 && (KMAX / G::KK) % 4 == 0 && 2 * ((PCH + 15) / 16) <= 16 && (PCH % 16 == 0 || PCH >= G::P) && G::P > 16;
};
// 80 positions (4 output rows) per workgroup: 5 x 96 = 480 workgroups at batch 32, one round at two per CU
// (64 positions gave 672, the seventh chunk of each image nearly empty: 224.4 vs 222.6 us per step; 100 positions
// = 384 workgroups measured 225)
struct CfgC1 : ConvCfg<GeomC1, 3, 20, 256, true, 80> { static constexpr const char* name = "GeomC1"; };
struct CfgC2 : ConvCfg<GeomC2, 3, 20, 512, false> { static constexpr const char* name = "GeomC2"; };
struct CfgC3 : ConvCfg<GeomC3, 2, 9, 576, false> { static constexpr const char* name = "GeomC3"; };
struct CfgD1 : ConvCfg<GeomD1, 2, 20, 100, true> { static constexpr const char* name = "GeomD1"; };
struct CfgD2 : ConvCfg<GeomD2, 1, 16, 800, false> { static constexpr const char* name = "GeomD2"; };

// THE geometry ladder: f(Cfg{}) for the geometry of conv layer c
template <class F>
static auto with_geom(const ConvLayer& c, F&& f) -> decltype(f(CfgC1{})) {
  if (c.ks == 8) return f(CfgC1{});
  if (c.ks == 4) return f(CfgC2{});
  if (c.ks == 3) return f(CfgC3{});
  if (c.ih == 84) return f(CfgD1{});
  return f(CfgD2{});
}

// Image-group-fastest block order wants a group count that is a multiple of 8 — and the same groups as the next layer's launch and
// the weight-gradient launch (8 images each at batch 256), so that a group's dY stays in one XCD's L2 down the chain: the smallest
// images-per-workgroup count >= ipb that divides the batch into a multiple of 8 groups (the batch itself when there is none)
static int round_ipb_to_groups_of_8(int B, int ipb) {
  while (ipb < B && (rb_div_up(B, ipb) % 8 != 0 || B % ipb != 0)) ++ipb;
  return ipb;
}

// ----------------------------------------------------------------- conv forward --
enum ConvFwdKernel { CONV_FWD_GEMM, CONV_FWD_FULL, CONV_FWD_MULTI_T16, CONV_FWD_T16, CONV_FWD_LDS, CONV_FWD_LDS_F32 };
static const char* const conv_fwd_kernel_name[] = {"k_gemm", "k_conv_fwd_full", "k_conv_fwd_multi_t16", "k_conv_fwd_t16", "k_conv_fwd_lds",
                                                   "k_conv_fwd_lds"};
struct ConvFwdPlan {
  ConvFwdKernel kernel;
  dim3 grid;
  unsigned block;
  int ipb, img_fast;      // images per workgroup; image(-group)-fastest block order
  const char* geom;
};
template <class C>
static ConvFwdPlan plan_conv_fwd_g(const PlanIn& in, int layer, int n_on, int n_tg, bool f32) {
  using G = typename C::G;
  const ConvLayer& c = in.L.conv[layer];
  const int NI = n_on + n_tg;
  ConvFwdPlan p;
  p.ipb = 1; p.img_fast = 0; p.geom = C::name;
  if (!in.caps.fast_conv) {      // gemm_core.h: 64 positions per block for the first layer, 32 behind it
    const int n_max = (n_on > n_tg ? n_on : n_tg) * G::P;
    p.kernel = CONV_FWD_GEMM; p.grid = dim3(1, (unsigned)rb_div_up(n_max, layer == 0 ? 64 : 32), 2); p.block = 128;
    return p;
  }
  const bool out_blocked = layer == in.L.nconv - 1 && in.caps.fast_fc;
  // large batches: one round of workgroups, each keeping its weight slab for ipb images of one net (conv_fwd_multi.h, conv_fwd_full.h)
  const bool multi_forced = in.opt.conv_multi >= 0;
  int ipb = 0;
  if (multi_forced) ipb = in.opt.conv_multi;
  else if (NI >= 256) {
    const int per_img = (int)(rb_div_up(G::P, C::PCH) * rb_div_up(c.cout, 32));
    ipb = (int)rb_div_up((int64_t)NI * per_img, 256);
  }
  if constexpr (C::FIRST && ConvFwdFullLds<G, C::KMAX>::FITS) {
    // first layer: whole image per workgroup, whole reduction per wave
    if (ipb > 0 && !f32 && c.cout <= 32 && !out_blocked && in.opt.conv_full && c.cin * G::KK == C::KMAX && (C::KMAX & 1) == 0) {
      int fi = ipb;
      if (!multi_forced) fi = (int)rb_div_up(NI, 256);         // one round of workgroups
      p.kernel = CONV_FWD_FULL; p.ipb = fi; p.grid = dim3(1, 1, (unsigned)rb_div_up(NI, fi)); p.block = RB_CONV_THREADS;
      return p;
    }
  }
  if constexpr (!C::FIRST && C::T16_OK) {      // (first layers: k_conv_fwd_full above)
    if (ipb > 0) {
      const unsigned ngroups = (unsigned)rb_div_up(NI, ipb);
      p.kernel = CONV_FWD_MULTI_T16; p.ipb = ipb;
      p.grid = dim3((unsigned)rb_div_up(G::P, C::PCH), (unsigned)rb_div_up(c.cout, 32), ngroups);
      if (in.opt.img_fast && ngroups % 8 == 0) {     // image-group-fastest block order (layers 2 and 3 use the same ipb)
        p.img_fast = 1;
        p.grid = dim3(ngroups, (unsigned)rb_div_up(c.cout, 32), (unsigned)rb_div_up(G::P, C::PCH));
      }
      p.block = 64 * ConvFwdWaves<C::KMAX, C::PCH, true>::NWV;
      return p;
    }
  }
  p.grid = dim3((unsigned)rb_div_up(G::P, C::PCH), (unsigned)rb_div_up(c.cout, 32), (unsigned)NI);
  if (in.opt.img_fast && NI % 8 == 0) {     // image-fastest block order (XCD = image mod 8 in every layer)
    p.img_fast = 1;
    p.grid = dim3((unsigned)NI, (unsigned)rb_div_up(c.cout, 32), (unsigned)rb_div_up(G::P, C::PCH));
  }
  if constexpr (C::T16_OK) {
    // the first layer: u8 frames of a full history only (f32 states — act / evaluate — and history < 4 run the split-K kernel below)
    if (!C::FIRST || (in.opt.t16 && !f32 && c.cin * G::KK == C::KMAX)) {
      // (one channel tile per wave: 2 measured slower for the first layer — 5-wave staging)
      p.kernel = CONV_FWD_T16; p.block = 64 * ConvFwdWaves<C::KMAX, C::PCH, true>::NWV;
      return p;
    }
  }
  // split-K 32x32x2 tiles: first layers (above) and the data-efficient second layer; float states (act / evaluate) have an
  // instantiation of their own (conv_fwd_image.h F32SRC)
  p.kernel = (C::FIRST && f32) ? CONV_FWD_LDS_F32 : CONV_FWD_LDS; p.block = RB_CONV_THREADS;
  return p;
}
static ConvFwdPlan plan_conv_fwd(const PlanIn& in, int layer, int n_on, int n_tg, bool f32) {
  return with_geom(in.L.conv[layer], [&](auto cfg) { return plan_conv_fwd_g<decltype(cfg)>(in, layer, n_on, n_tg, f32); });
}

// ---------------------------------------------------------- conv input gradient --
// The data gradient of conv layer `layer` (>= 1) on the whole-K 16x16x4 tile kernel (conv_dx.h k_conv_dx_t16_multi): the image-loop
// form, i.e. batches of 64 and more (or RB_OPTS dx_ipb > 1, the test hook), the canonical later layers' geometries (64 output
// channels, kernel size a multiple of the stride); the data-efficient second layer's image loop is k_conv_dx_lds<..., MULTI>.
// Decides the layout of conv_wT too (the head launch's tenant jobs write it).
static constexpr bool dx_t16_geom(int ks, int s, int ih) { return (ks == 4 && s == 2 && ih == 20) || (ks == 3 && s == 1 && ih == 9); }   // GeomC2 / GeomC3
static bool dx_uses_t16(const PlanIn& in, int layer) {
  const Layout& L = in.L;
  if (layer < 1 || layer >= L.nconv || !in.caps.fast_conv || !in.caps.wT[layer]) return false;
  const ConvLayer& c = L.conv[layer];
  return dx_t16_geom(c.ks, c.s, c.ih) && (L.B >= 64 || in.opt.dx_ipb > 1);
}
// positions of one stride phase of the input, in 32-position tiles; few images at batch 32: spread each phase's positions over
// several workgroups (weights are re-staged from L2)
template <class G>
struct ConvDxTiles {
  static constexpr int NPOS = ((G::IH + G::S - 1) / G::S) * ((G::IH + G::S - 1) / G::S);
  static constexpr int NT_ALL = (NPOS + 31) / 32;
  static constexpr int NT = NT_ALL >= 4 ? 2 : 1;
};
enum ConvDxKernel { CONV_DX_NONE, CONV_DX_LDS, CONV_DX_LDS_MULTI, CONV_DX_T16_MULTI, CONV_DX_GEMM };
static const char* const conv_dx_kernel_name[] = {"none", "k_conv_dx_lds", "k_conv_dx_lds", "k_conv_dx_t16_multi", "k_gemm"};
struct ConvDxPlan {
  ConvDxKernel kernel;
  dim3 grid;
  unsigned block;
  int ipb, img_fast;
  int wt_t16;             // layout of conv_wT[layer] (ConvWtJob::t16)
  const char* geom;
};
template <class C>
static ConvDxPlan plan_conv_dx_g(const PlanIn& in, int layer, bool lazy_dfeat) {
  using G = typename C::G;
  const Layout& L = in.L;
  const ConvLayer& c = L.conv[layer];
  ConvDxPlan p;
  p.kernel = CONV_DX_NONE; p.grid = dim3(0, 0, 0); p.block = 0; p.ipb = 1; p.img_fast = 0; p.geom = C::name;
  p.wt_t16 = dx_uses_t16(in, layer) ? 1 : 0;
  if constexpr (G::IH == 84) {
    // first-layer geometries never need a data gradient (frames are not differentiated)
  } else if (layer > 0 && in.caps.fast_conv && in.caps.wT[layer] && ((lazy_dfeat && layer == L.nconv - 1) == RB_LAST_CONV_GEOM(G))) {
    // (the last layer's LDS kernel exists in its LAZY form only — dY summed from the hidden layer's row-split partials while
    // it is staged; when those are not what the step produced, i.e. the generic FC path ran, the generic kernel below runs)
    const unsigned groups = (unsigned)rb_div_up(ConvDxTiles<G>::NT_ALL, ConvDxTiles<G>::NT);
    // batches of 64 and more: about one round of workgroups over the chip, each keeping its weight slab for ipb images
    const int ipb_env = in.opt.dx_ipb;                                            // (1 = one image each)
    const int cit = (int)rb_div_up(c.cin, 32);
    if constexpr (dx_t16_geom(G::KS, G::S, G::IH)) {
      if (p.wt_t16) {
        // whole-K tiles: a workgroup per (phase, 32 input channels, image group), about one round of 256
        const int units = G::S * G::S * cit;
        int tp = ipb_env > 0 ? ipb_env : (int)rb_div_up((int64_t)units * L.B, 256);
        if (tp < 1) tp = 1;
        if (ipb_env <= 0 && in.opt.img_fast) tp = round_ipb_to_groups_of_8(L.B, tp);
        const unsigned ng = (unsigned)rb_div_up(L.B, tp);
        p.kernel = CONV_DX_T16_MULTI; p.ipb = tp;
        p.img_fast = (in.opt.img_fast && L.B % tp == 0 && ng % 8 == 0) ? 1 : 0;
        p.grid = p.img_fast ? dim3(ng, (unsigned)cit, (unsigned)(G::S * G::S)) : dim3((unsigned)(G::S * G::S), (unsigned)cit, ng);
        p.block = 64 * ConvDxT16<G, 64>::NWV;
        return p;
      }
    }
    const int per_img = (G::S * G::S) * (int)groups * cit;
    int ipb = 1;
    if (ipb_env > 0) ipb = ipb_env;
    else if (L.B >= 64) {                             // ONE round of workgroups (their LDS footprint allows one per CU)
      while (per_img * (int)rb_div_up(L.B, ipb) > 256) ++ipb;
      if (in.opt.img_fast) ipb = round_ipb_to_groups_of_8(L.B, ipb);
    }
    p.ipb = ipb;
    p.grid = dim3((unsigned)(G::S * G::S) * groups, (unsigned)cit, (unsigned)rb_div_up(L.B, ipb));
    if (in.opt.img_fast && L.B % ipb == 0 && (L.B / ipb) % 8 == 0) {      // image(-group)-fastest block order: image i on XCD i mod 8 in every conv launch
      p.img_fast = 1;
      p.grid = dim3((unsigned)(L.B / ipb), (unsigned)cit, (unsigned)(G::S * G::S) * groups);
    }
    // (the canonical geometries' image loop is the t16 kernel above: their k_conv_dx_lds has no MULTI instantiation)
    p.kernel = (!dx_t16_geom(G::KS, G::S, G::IH) && ipb > 1) ? CONV_DX_LDS_MULTI : CONV_DX_LDS;
    p.block = RB_CONV_THREADS;
  } else if (layer > 0) {
    const int nyy = (G::IH + G::S - 1) / G::S;
    const int n_max = L.B * nyy * nyy;
    p.kernel = CONV_DX_GEMM; p.block = 128;
    p.grid = c.cin <= 32 ? dim3(1, (unsigned)rb_div_up(n_max, 64), (unsigned)(G::S * G::S))
                         : dim3((unsigned)rb_div_up(c.cin, 64), (unsigned)rb_div_up(n_max, 32), (unsigned)(G::S * G::S));
  }
  return p;
}
static ConvDxPlan plan_conv_dx(const PlanIn& in, int layer, bool lazy_dfeat) {
  return with_geom(in.L.conv[layer], [&](auto cfg) { return plan_conv_dx_g<decltype(cfg)>(in, layer, lazy_dfeat); });
}

// --------------------------------------------------------- conv weight gradients --
// every layer in one launch (LDS kernels)
struct ConvDwAllPlan {
  int ipb[3], cotiles[3], nblocks[3], dw_slices[3];
  int img_fast;
  unsigned total;
};
static ConvDwAllPlan plan_conv_dw_all(const PlanIn& in) {
  const Layout& L = in.L;
  ConvDwAllPlan p;
  memset(&p, 0, sizeof(p));
  const int ipb_all = L.B > 32 ? (int)rb_div_up(L.B, 32) : 1;      // keep about 32 image groups: the slice count stays at its batch-32 size
  bool uniform = true;
  for (int i = 0; i < 3; ++i) p.ipb[i] = ipb_all;
  // Batches beyond 32, the canonical stack: images per workgroup chosen PER LAYER.  A workgroup walks its images one after the other
  // and the layers' images cost differently (7.5 / 7.4 / 6.2 us per image at batch 256, tools/wg_timeline.py): with 8 images
  // everywhere the launch was 224 workgroups of 60 / 59 / 50 us on 256 CUs; 7 / 7 / 8 images are 249 workgroups of 52 / 52 / 50 us
  // (-7.6 us per step, profiles/round6_dw_layer_ipb_ab.txt).  Smallest longest workgroup that still fits ONE round over the CUs.
  if (L.B > 32 && L.nconv == 3) {
    const int cost[3] = {75, 74, 62};
    const int chunks0 = (L.conv[0].oh + 6) / 7, ct[3] = {(int)rb_div_up(L.conv[0].cout, 32), (int)rb_div_up(L.conv[1].cout, 32), (int)rb_div_up(L.conv[2].cout, 32)};
    int best_t = ipb_all * cost[0], best[3] = {ipb_all, ipb_all, ipb_all};
    for (int i0 = 1; i0 <= ipb_all; ++i0)
      for (int i1 = 1; i1 <= ipb_all + 4; ++i1)
        for (int i2 = 1; i2 <= ipb_all + 4; ++i2) {
          const int wgs = chunks0 * ct[0] * (int)rb_div_up(L.B, i0) + ct[1] * (int)rb_div_up(L.B, i1) + ct[2] * (int)rb_div_up(L.B, i2);
          if (wgs > in.n_cu) continue;
          int t = i0 * cost[0];
          if (i1 * cost[1] > t) t = i1 * cost[1];
          if (i2 * cost[2] > t) t = i2 * cost[2];
          if (t < best_t) { best_t = t; best[0] = i0; best[1] = i1; best[2] = i2; }
        }
    for (int i = 0; i < 3; ++i) p.ipb[i] = best[i];
  }
  const int dw_ipb[3] = {in.opt.dw_ipb0, in.opt.dw_ipb1, in.opt.dw_ipb2};
  for (int i = 0; i < L.nconv; ++i) {
    if (dw_ipb[i] > 0) p.ipb[i] = dw_ipb[i];
    if (p.ipb[i] > L.B) p.ipb[i] = L.B;
    if (p.ipb[i] != ipb_all) uniform = false;
    const int groups = (int)rb_div_up(L.B, p.ipb[i]);
    const ConvLayer& c = L.conv[i];
    // first layer: 7-row chunks (3 per image) so that all layers together are 96 + 64 + 64 = 224 workgroups at batch 32,
    // ONE round over the 256 CUs (5-row chunks gave 288 workgroups at one per CU: a second round for 32 of them)
    const int rc = i == 0 ? (c.ks == 8 ? 7 : 4) : c.oh;                 // later layers: the whole image is one chunk
    const int chunks = (c.oh + rc - 1) / rc;
    p.cotiles[i] = (int)rb_div_up(c.cout, 32);
    p.nblocks[i] = chunks * p.cotiles[i] * groups;
    p.dw_slices[i] = chunks * groups;
    p.total += (unsigned)p.nblocks[i];
  }
  for (int i = L.nconv; i < 3; ++i) { p.nblocks[i] = 0; p.cotiles[i] = 1; }
  // image-fastest decode (an image group's workgroups of every layer on XCD group mod 8, where the input-gradient chain left
  // its dY): block ranges and the group count must be multiples of 8
  p.img_fast = (in.opt.img_fast && uniform && (int)rb_div_up(L.B, ipb_all) % 8 == 0 && p.nblocks[0] % 8 == 0 && p.nblocks[1] % 8 == 0) ? 1 : 0;
  return p;
}
// one layer on the gemm_core.h fallback (split-K slices, summed by k_reduce_conv_dw_all)
struct ConvDwGemmPlan { dim3 grid; unsigned block; int splits; };
static ConvDwGemmPlan plan_conv_dw_gemm(const PlanIn& in, int layer) {
  const ConvLayer& c = in.L.conv[layer];
  ConvDwGemmPlan p;
  p.splits = in.caps.ws[layer];
  p.grid = dim3((unsigned)rb_div_up(c.cout, layer == 0 ? 32 : 64), (unsigned)rb_div_up(c.K() + 1, 64), (unsigned)p.splits);
  p.block = layer == 0 ? 128 : 256;
  return p;
}

// ------------------------------------------------------------------- FC layers --
// From 128 rows per net on the hidden layer is a GEMM, not a weight stream: 128 x 128 LDS tiles (fc_gemm.h).  `rows` = the rows
// of the larger net THIS launch sees: the forward's online net carries states AND next_states (2B rows), the backward B.  So at
// B = 64 ... 127 the forward runs k_fc_gemm_fwd while the backward stays on k_nl_bwd — on purpose: each side switches where
// ITS row count makes the tiled kernel pay.
static bool fc_uses_gemm(const PlanIn& in, int rows) {
  return in.caps.gemm_ws && (in.opt.fc_gemm == 1 || (in.opt.fc_gemm < 0 && rows >= 128));
}
enum FcFwdKernel { FC_FWD_KGEMM, FC_FWD_NL3_2, FC_FWD_NL3_4, FC_FWD_TILED };
static const char* const fc_fwd_kernel_name[] = {"k_gemm", "k_nl_fwd3<2>", "k_nl_fwd3<4>", "k_fc_gemm_fwd"};
struct FcFwdPlan {
  FcFwdKernel h_kernel, z_kernel;
  dim3 hgrid, zgrid;
  unsigned hblock, zblock;
  int block_copy;               // the generic conv path fed the streamed FC kernels: k_block_copy first
  int mt[2], nt, tiles, S;      // k_fc_gemm_fwd: 128-row tiles per net, column tiles, tile count, split-K factor
};
static FcFwdPlan plan_fc_fwd(const PlanIn& in, int n_on, int n_tg) {
  const Layout& L = in.L;
  FcFwdPlan p;
  memset(&p, 0, sizeof(p));
  const int m_max = n_on > n_tg ? n_on : n_tg;
  if (!in.caps.fast_fc) {
    p.h_kernel = p.z_kernel = FC_FWD_KGEMM;
    p.hgrid = dim3((unsigned)rb_div_up(m_max, 64), (unsigned)rb_div_up(2 * L.H, 64), (unsigned)(2 * in.caps.hs)); p.hblock = 256;
    p.zgrid = dim3((unsigned)rb_div_up(m_max, 32), (unsigned)rb_div_up(L.NZ - L.Z, 32), 4); p.zblock = 64;
    return p;
  }
  p.block_copy = in.caps.fast_conv ? 0 : 1;
  const int ht16 = (int)rb_div_up(L.H, 16);
  // batch 256: 64-row m-chunks halve the passes over the weights (at batch 32 one 64-row chunk for the online net's rows
  // reads every tile once instead of twice and is 7 us per step SLOWER: a workgroup's MFMAs are serial on its CU)
  const bool wide = m_max >= 128;
  const unsigned mch32 = (unsigned)rb_div_up(m_max, wide ? 64 : RB_NL_FWD_MROWS);
  // (16-row m-chunks — 384 workgroups, every CU busy — measured 20.8 us against 16.2: the tiles are re-read four times)
  p.hgrid = dim3((unsigned)(2 * ht16), 1, 2 * mch32); p.hblock = 64 * RB_NL_FWD_WAVES;
  p.h_kernel = wide ? FC_FWD_NL3_4 : FC_FWD_NL3_2;
  if (fc_uses_gemm(in, m_max)) {      // split-K over the idle CUs
    p.mt[0] = (int)rb_div_up(n_on, RB_TG_T); p.mt[1] = (int)rb_div_up(n_tg, RB_TG_T);
    p.nt = (int)rb_div_up(2 * L.H, RB_TG_T);
    p.tiles = (p.mt[0] + p.mt[1]) * p.nt;
    int S = in.n_cu / p.tiles;
    if (S > 8) S = 8;
    if (S > L.F / RB_TG_KS) S = L.F / RB_TG_KS;
    if (S < 1 || p.tiles > 1024) S = 1;
    p.S = S;
    p.h_kernel = FC_FWD_TILED; p.hgrid = dim3((unsigned)(p.tiles * S)); p.hblock = RB_TG_THREADS;
  }
  // output layer: value rows read h[:, :H], advantage rows read h[:, H:]
  const int vt16 = (int)rb_div_up(L.Z, 16), at16 = (int)rb_div_up(L.NZ - L.Z, 16);
  p.z_kernel = wide ? FC_FWD_NL3_4 : FC_FWD_NL3_2;
  p.zgrid = dim3((unsigned)(vt16 + at16), 1, 2 * mch32); p.zblock = 64 * RB_NL_FWD_WAVES;
  return p;
}

// The noisy layers of rb_learner_act_batch_rows (noisy_rows.h: one noise sample per row, n <= 256 rows of the online net): the
// streamed two-contraction kernel where k_nl_fwd3's preconditions hold, in 16-row m-chunks up to 16 rows and 32-row ones beyond (its
// accumulators and reduction buffer are twice fwd3's: no 64-row form); else one wave per output cell.  The scaled-copy pass in front
// of the streamed hidden layer always runs (it also writes feat_b, whichever conv path produced the features).
enum ActRowsKernel { ACT_ROWS_NLR_1, ACT_ROWS_NLR_2, ACT_ROWS_GENERIC };
static const char* const act_rows_kernel_name[] = {"k_nlr_fwd<1>", "k_nlr_fwd<2>", "k_nlr_generic"};
struct ActRowsPlan {
  ActRowsKernel kernel;
  dim3 copy_grid, hgrid, zgrid;     // copy_grid.x == 0: no scaled-copy pass (the fallback reads eps_in in place)
  unsigned block;
};
static ActRowsPlan plan_act_rows(const PlanIn& in, int n) {
  const Layout& L = in.L;
  ActRowsPlan p;
  memset(&p, 0, sizeof(p));
  if (!in.caps.fast_fc) {
    p.kernel = ACT_ROWS_GENERIC; p.block = 256;
    p.copy_grid = dim3(0, 1, 1);
    p.hgrid = dim3((unsigned)rb_div_up((int64_t)n * 2 * L.H, 4));
    p.zgrid = dim3((unsigned)rb_div_up((int64_t)n * L.NZ, 4));
    return p;
  }
  const int mt = n <= 16 ? 1 : 2;
  p.kernel = mt == 1 ? ACT_ROWS_NLR_1 : ACT_ROWS_NLR_2; p.block = 64 * RB_NL_FWD_WAVES;
  const unsigned mch = (unsigned)rb_div_up(n, 16 * mt);
  p.copy_grid = dim3((unsigned)rb_div_up((int64_t)n * L.F, 256));
  p.hgrid = dim3((unsigned)(2 * rb_div_up(L.H, 16)), 1, mch);
  p.zgrid = dim3((unsigned)(rb_div_up(L.Z, 16) + rb_div_up(L.NZ - L.Z, 16)), 1, mch);
  return p;
}

// tiles of the weight-gradient problem of one noisy layer pair (which = 0: fc_z_v | fc_z_a, 1: fc_h_v | fc_h_a); ct > 0 selects the
// pipelined body (M <= 32) with ct 256-column tiles per wave.  slots = sum-of-squares partials the launch writes.
struct FcDwTiles { int dw_x, dw_y, slots; };
static FcDwTiles plan_fc_dw_tiles(const Layout& L, int which, int ct) {
  FcDwTiles t;
  const int K = which == 0 ? L.H : L.F;
  t.dw_y = which == 0 ? (int)rb_div_up(L.Z, 16) + (int)rb_div_up(L.NZ - L.Z, 16) : 2 * (int)rb_div_up(L.H, 16);
  t.dw_x = (int)rb_div_up(K, 256 * (ct > 0 ? ct : 1));
  t.slots = 4 * t.dw_x * t.dw_y;
  return t;
}

enum FcBwdKernel { FC_BWD_KGEMM, FC_BWD_NL_TALL, FC_BWD_NL, FC_BWD_TILED, FC_BWD_NONE };
static const char* const fc_bwd_kernel_name[] = {"k_gemm", "k_nl_bwd<true>", "k_nl_bwd<false>", "k_fc_gemm_bwd", "none"};
struct FcBwdPlan {
  FcBwdKernel z_kernel, h_kernel;
  bool exch;
  bool pipe;                   // pipelined weight-gradient body (one reduction pass per tile, i.e. batch <= 32)
  int z_ct, h_ct;              // ... with this many 256-column tiles per wave and workgroup
  bool gemm_bwd;               // the hidden layer's two gradients as LDS-tiled GEMMs in one launch (fc_gemm.h k_fc_gemm_bwd)
  bool fuse_norm;              // the launches leave the gradient's sum of squares in norm_part (no k_sumsq pass)
  bool defer_dw;               // RB_LEARNER_FUSE_FC_H_DW: the hidden layer's weight gradient for its norm only
  bool implicit_sigma;         // RB_LEARNER_IMPLICIT_SIGMA: g_sigma of the hidden layer left to the optimiser pass
  FcDwTiles z, h;
  int c_slots, norm_slots, norm_conv_base;    // slots: [fc_z dW waves | fc_h dW waves | conv reduce blocks]
  int rows_per_split, hsplits;                // row splits of the hidden layer's input gradient
  bool z_tall;                 // the output layer's input gradient with eight waves per workgroup (batch <= 32)
  bool up_enabled;             // the priority write-back rides in the hidden layer's launch
  bool lazy_dfeat;             // the last conv layer's backward kernels sum the dfeat partials themselves (no k_dfeat_finish)
  bool pack;                   // replica exchange: k_pack_factors between the two launches
  NlBwdGrid zg, hg;
  FcGemmBwdGrid gg;
  int g_nt, g_kt;
  unsigned z_blocks, z_threads, h_blocks, h_threads;
  dim3 gz_dw, gz_dx, gh_dw, gh_dx;            // the gemm_core.h fallback's four launches
};
// spec: this call's write-back leaves for the replay's stream (the early draw; decided per call)
static FcBwdPlan plan_fc_bwd(const PlanIn& in, bool spec) {
  const Layout& L = in.L;
  const int B = L.B;
  FcBwdPlan p;
  memset(&p, 0, sizeof(p));
  if (!in.caps.fast_fc) {
    p.z_kernel = p.h_kernel = FC_BWD_KGEMM;
    p.gz_dw = dim3((unsigned)rb_div_up(L.NZ - L.Z, 32), (unsigned)rb_div_up(L.H + 1, 64), 2);
    p.gz_dx = dim3((unsigned)rb_div_up(B, 32), (unsigned)rb_div_up(L.H, 32), 2);
    p.gh_dw = dim3((unsigned)rb_div_up(2 * L.H, 64), (unsigned)rb_div_up(L.F + 1, 64), 1);
    p.gh_dx = dim3((unsigned)rb_div_up(B, 32), (unsigned)rb_div_up(L.F, 64), (unsigned)in.caps.xs);
    p.hsplits = in.caps.xs;
    return p;
  }
  const bool exch = in.exch;
  p.exch = exch; p.pack = exch;
  p.pipe = B <= 32 && !exch;
  p.z_ct = p.pipe ? 2 : 0; p.h_ct = p.pipe ? 4 : 0;
  p.z = plan_fc_dw_tiles(L, 0, p.z_ct);
  p.h = plan_fc_dw_tiles(L, 1, p.h_ct);
  // batch >= 128 (fc_uses_gemm sees the backward's B rows)
  p.gemm_bwd = !exch && fc_uses_gemm(in, B);
  p.g_nt = (int)rb_div_up(2 * L.H, RB_TG_T); p.g_kt = (int)rb_div_up(L.F, RB_TG_T);
  if (p.gemm_bwd) p.h.slots = 8 * p.g_nt * p.g_kt;             // one sum-of-squares slot per wave of a weight-gradient tile
  int64_t conv_out = 0;
  for (int layer = 0; layer < L.nconv; ++layer) conv_out += (int64_t)L.conv[layer].cout * (L.conv[layer].K() + 1);
  p.c_slots = (int)rb_div_up(conv_out, 64);
  p.fuse_norm = !exch && p.z.slots + p.h.slots + p.c_slots <= RB_NORM_PART_SLOTS;
  p.defer_dw = (in.flags & RB_LEARNER_FUSE_FC_H_DW) && p.pipe && p.h_ct > 0 && p.fuse_norm && in.caps.fast_conv;
  // RB_LEARNER_IMPLICIT_SIGMA: g_sigma = g_mu * (eps_out x eps_in) is left to the optimiser pass (its square still enters
  // the norm here).  Needs the pipelined weight-gradient body (batch <= 32) or the tiled GEMM (batch >= 128), the fused norm and
  // adjacent mu | sigma arrays
  p.implicit_sigma = (in.flags & RB_LEARNER_IMPLICIT_SIGMA) && ((p.pipe && p.h_ct > 0) || p.gemm_bwd) && p.fuse_norm && !p.defer_dw &&
                     L.h_sigma == L.h_mu + (int64_t)2 * L.H * L.F && (L.F % 4) == 0 && (L.h_mu % 4) == 0 &&
                     ((int64_t)2 * L.H * L.F >= ((int64_t)1 << 20) || in.opt.implicit_small);   // (the data-efficient
                     // net's 0.3 M-element layer: +0.8 us per step with the pairing — it pays from megabytes on)
  p.norm_slots = p.fuse_norm ? p.z.slots + p.h.slots + p.c_slots : 0;
  p.norm_conv_base = p.z.slots + p.h.slots;
  const int vt = (int)rb_div_up(L.Z, 16), at = (int)rb_div_up(L.NZ - L.Z, 16);
  // the output layer's input gradient with eight waves per workgroup (nl_dx.h rb_nl_dx_body_tall) at batch <= 32
  // on 32-column tiles (H % 32 == 0: fast_fc): twice the workgroups, half the weight bytes through each CU
  p.z_tall = B <= 32;
  p.zg = NlBwdGrid{exch ? 0 : p.z.dw_x, exch ? 0 : vt + at, (int)rb_div_up(L.H, p.z_tall ? 32 : 64), 1, 2 * (int)rb_div_up(B, 64),
                   p.z_tall ? RB_NL_DX_TALL : RB_NL_DX_M64_ST8};
  p.z_kernel = p.z_tall ? FC_BWD_NL_TALL : FC_BWD_NL;
  p.z_blocks = (unsigned)(p.zg.dw_x * p.zg.dw_y + p.zg.dx_x * p.zg.dx_y * p.zg.dx_z);
  p.z_threads = p.z_tall ? 64 * RB_NL_DXT_WAVES : 256;
  // ---- hidden layer
  p.rows_per_split = (int)rb_div_up(rb_div_up(2 * L.H, in.caps.xs), 16) * 16;
  p.hsplits = (int)rb_div_up(2 * L.H, p.rows_per_split);
  p.hg = NlBwdGrid{exch ? 0 : p.h.dw_x, exch ? 0 : p.h.dw_y, (int)rb_div_up(L.F, 64), p.hsplits, (int)rb_div_up(B, 64),
                   B <= 32 ? RB_NL_DX_M32_ST8 : RB_NL_DX_M64_ST4};
  p.up_enabled = in.sink && B <= 256 && !spec;
  // the priority write-back (a single-workgroup latency chain of ~11 us) rides in the LONGER of the two backward
  // launches: as a tenant of the output layer's launch (~8 us of real work) it was that launch's long pole
  p.h_blocks = (unsigned)(p.hg.dw_x * p.hg.dw_y + p.hg.dx_x * p.hg.dx_y * p.hg.dx_z + (p.up_enabled ? 1 : 0));
  p.h_threads = 256;
  p.h_kernel = p.h_blocks > 0 ? FC_BWD_NL : FC_BWD_NONE;
  if (p.gemm_bwd) {
    FcGemmBwdGrid& gg = p.gg;
    gg.first = p.up_enabled ? 8 : 0;
    gg.dx_mt = (int)rb_div_up(B, RB_TG_T); gg.dx_kt = p.g_kt; gg.dx_splits = p.hsplits;
    gg.dx_combos = (int)rb_div_up(p.g_kt * p.hsplits, 8) * 8;
    gg.dw_nt = p.g_nt; gg.dw_kt = p.g_kt;
    p.h_kernel = FC_BWD_TILED;
    p.h_blocks = (unsigned)(gg.first + gg.dx_mt * gg.dx_combos + p.g_nt * p.g_kt);
    p.h_threads = RB_TG_THREADS;
  }
  // d(conv output) = relu' * sum of the row-split partials: formed by its two consumers (the last conv layer's dX and
  // dW kernels) while they stage it, instead of a ~5 us launch of its own between two dependent kernels
  p.lazy_dfeat = in.caps.fast_conv && L.nconv >= 2 && p.hsplits <= 4;
  return p;
}

// ------------------------------------------------------------------------- head --
struct HeadPlan {
  int ZI;                 // atom slots per lane: the k_head<ZI> instantiation (ceil(Z / 64) rounded to 1, 2 or 4)
  int waves;              // one wave per softmax task (2A + 1) up to 16 waves, at least 8 (the logits sweep and the dlogits store want lanes)
  int n_jobs, job_layer[2], job_t16[2];     // tenant jobs: conv_wT of these layers, in this layout
  int per_job;            // workgroups per job (one element or two per thread: the tenants must stay shorter than the head)
  unsigned blocks;
};
static HeadPlan plan_head(const PlanIn& in) {
  const Layout& L = in.L;
  HeadPlan p;
  memset(&p, 0, sizeof(p));
  p.ZI = L.Z <= 64 ? 1 : (L.Z <= 128 ? 2 : 4);
  p.waves = 2 * L.A + 1;
  if (p.waves < 8) p.waves = 8;
  if (p.waves > 16) p.waves = 16;
  if (in.caps.fast_conv) {
    for (int layer = 1; layer < L.nconv && p.n_jobs < 2; ++layer) {
      if (!in.caps.wT[layer]) continue;
      p.job_layer[p.n_jobs] = layer; p.job_t16[p.n_jobs] = dx_uses_t16(in, layer) ? 1 : 0;
      ++p.n_jobs;
    }
    p.per_job = p.n_jobs > 0 ? 48 : 0;
  }
  p.blocks = (unsigned)(L.B + (p.n_jobs > 0 ? 2 * p.per_job : 0));
  return p;
}

// one fixed-order reduction of every conv layer's split slices (64 outputs per block); snapshot: tenant blocks behind them copy the
// learn call's online noise for the optimiser pass that forms the hidden layer's sigma gradient itself
static unsigned plan_conv_reduce_blocks(const Layout& L, bool snapshot) {
  int64_t total = 0;
  for (int layer = 0; layer < L.nconv; ++layer) total += (int64_t)L.conv[layer].cout * (L.conv[layer].K() + 1);
  return (unsigned)(rb_div_up(total, 64) + (snapshot ? rb_div_up((int)L.n_noise, 64) : 0));
}

// -------------------------------------------------------------- clip without partials --
// The gradient came from the fallback path or was modified since (all-reduce): blocks of the one k_sumsq pass over it
static int plan_sumsq_blocks(int64_t n) {
  int nblocks = (int)rb_div_up(n, 256 * 16);
  if (nblocks > 1024) nblocks = 1024;
  return nblocks;
}
