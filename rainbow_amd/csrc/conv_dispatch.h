// conv_dispatch.h — the conv launches of the learner: take the plan (learner_plan.h), fill the argument struct, switch on the
// kernel id to the template instantiation.  Included by learner.hip only.
#pragma once
#include "learner_plan.h"

static PlanIn plan_in(const rb_learner* l) {
  return PlanIn{l->L, l->opt, l->caps, l->n_cu, l->flags, l->world > 1 && l->fact_local != nullptr && l->caps.fast_fc, l->sink != nullptr};
}

template <class C>
static int launch_conv_fwd(rb_learner* l, int layer, int n_on, int n_tg, const ImgSrc& src, const NetPtrs& on,
                           const NetPtrs& tg, hipStream_t stream) {
  using G = typename C::G;
  constexpr int NT = C::NT, PR = C::PR, KMAX = C::KMAX, PCH = C::PCH;
  constexpr bool FIRST = C::FIRST;
  const ConvLayer& c = l->L.conv[layer];
  const ConvFwdPlan p = plan_conv_fwd_g<C>(plan_in(l), layer, n_on, n_tg, src.f32 != nullptr);
  if (p.kernel == CONV_FWD_GEMM) {
    if (layer == 0) {
      ConvFwdProb<G, true> q;
      q.cin = c.cin; q.cout = c.cout;
      q.n_img[0] = n_on; q.n_img[1] = n_tg; q.img_base[0] = 0; q.img_base[1] = n_on;
      q.w[0] = on.conv_w[0]; q.w[1] = tg.conv_w[0]; q.bias[0] = on.conv_b[0]; q.bias[1] = tg.conv_b[0];
      q.src = src; q.in_f = nullptr; q.out = l->act[0];
      RB_LAUNCH((k_gemm<1, 2, ConvFwdProb<G, true>>), p.grid, dim3(p.block), stream, q);
    } else {
      ConvFwdProb<G, false> q;
      q.cin = c.cin; q.cout = c.cout;
      q.n_img[0] = n_on; q.n_img[1] = n_tg; q.img_base[0] = 0; q.img_base[1] = n_on;
      q.w[0] = on.conv_w[layer]; q.w[1] = tg.conv_w[layer]; q.bias[0] = on.conv_b[layer]; q.bias[1] = tg.conv_b[layer];
      q.src = src; q.in_f = l->act[layer - 1]; q.out = l->act[layer];
      RB_LAUNCH((k_gemm<2, 1, ConvFwdProb<G, false>>), p.grid, dim3(p.block), stream, q);
    }
    RB_LAUNCH_CHECK();
    return RB_OK;
  }
  ConvLdsFwdArgs a;
  a.cin = c.cin; a.cout = c.cout; a.n_on = n_on;
  a.w[0] = on.conv_w[layer]; a.w[1] = tg.conv_w[layer]; a.bias[0] = on.conv_b[layer]; a.bias[1] = tg.conv_b[layer];
  a.src = src; a.in_f = layer > 0 ? l->act[layer - 1] : nullptr; a.out = l->act[layer];
  a.out_blocked = (layer == l->L.nconv - 1 && l->caps.fast_fc) ? l->feat_b : nullptr;
  a.rows_total = n_on + n_tg;
  a.ipb = p.ipb;
  a.img_fast = p.img_fast;
  static const char* const tags[3] = {"conv1_fwd:k_conv_fwd_lds", "conv2_fwd:k_conv_fwd_lds", "conv3_fwd:k_conv_fwd_lds"};
  const dim3 block(p.block);
  switch (p.kernel) {      // (a geometry has the instantiations its plan can name, and no others)
    case CONV_FWD_FULL:
      if constexpr (FIRST && ConvFwdFullLds<G, KMAX>::FITS) { RB_LAUNCH_T(tags[layer], (k_conv_fwd_full<G, KMAX>), p.grid, block, stream, a); }
      break;
    case CONV_FWD_MULTI_T16:
      if constexpr (!FIRST && C::T16_OK) { RB_LAUNCH_T(tags[layer], (k_conv_fwd_multi_t16<G, NT, PR, KMAX, PCH>), p.grid, block, stream, a); }
      break;
    case CONV_FWD_T16:
      if constexpr (C::T16_OK) { RB_LAUNCH_T(tags[layer], (k_conv_fwd_t16<G, NT, PR, KMAX, FIRST, PCH>), p.grid, block, stream, a); }
      break;
    case CONV_FWD_LDS_F32:
      if constexpr (FIRST) { RB_LAUNCH_T(tags[layer], (k_conv_fwd_lds<G, NT, PR, KMAX, FIRST, PCH, FIRST>), p.grid, block, stream, a); }
      break;
    case CONV_FWD_LDS:
      if constexpr (FIRST || !C::T16_OK) { RB_LAUNCH_T(tags[layer], (k_conv_fwd_lds<G, NT, PR, KMAX, FIRST, PCH>), p.grid, block, stream, a); }
      break;
    case CONV_FWD_GEMM: break;
  }
  RB_LAUNCH_CHECK();
  return RB_OK;
}

static int conv_fwd(rb_learner* l, int layer, int n_on, int n_tg, const ImgSrc& src, const NetPtrs& on,
                    const NetPtrs& tg, hipStream_t stream) {
  return with_geom(l->L.conv[layer], [&](auto cfg) { return launch_conv_fwd<decltype(cfg)>(l, layer, n_on, n_tg, src, on, tg, stream); });
}

// the input gradient of conv layer `layer` into dact[layer - 1]
template <class C>
static int launch_conv_dx(rb_learner* l, int layer, hipStream_t stream) {
  using G = typename C::G;
  const Layout& L = l->L;
  const ConvLayer& c = L.conv[layer];
  const ConvDxPlan p = plan_conv_dx_g<C>(plan_in(l), layer, l->lazy_dfeat != 0);
  if (p.kernel == CONV_DX_NONE) return RB_OK;
  if constexpr (G::IH != 84) {
    if (p.kernel == CONV_DX_GEMM) {
      ConvDxProb<G> q;
      q.B = L.B; q.cin = c.cin; q.cout = c.cout;
      q.w = l->p_online + L.conv_w[layer]; q.dy = l->dact[layer]; q.x_act = l->act[layer - 1]; q.dx = l->dact[layer - 1];
      if (c.cin <= 32) { RB_LAUNCH((k_gemm<1, 2, ConvDxProb<G>>), p.grid, dim3(p.block), stream, q); }
      else { RB_LAUNCH((k_gemm<2, 1, ConvDxProb<G>>), p.grid, dim3(p.block), stream, q); }
      RB_LAUNCH_CHECK();
      return RB_OK;
    }
    ConvLdsDxArgs a;
    a.cin = c.cin; a.cout = c.cout;
    a.w = l->p_online + L.conv_w[layer]; a.dy = l->dact[layer]; a.x_act = l->act[layer - 1]; a.dx = l->dact[layer - 1];
    a.wT = l->conv_wT[layer];
    constexpr bool lazy = RB_LAST_CONV_GEOM(G);
    a.dy_part = l->dfeat_part; a.dy_mask = l->act[layer]; a.dy_stride = (int64_t)L.B * L.F; a.dy_splits = lazy ? l->lazy_splits : 0;
    a.ipb = p.ipb; a.batch = L.B; a.img_fast = p.img_fast;
    constexpr int NT = ConvDxTiles<G>::NT;
    static const char* const tags[3] = {"conv1_dx:k_conv_dx_lds", "conv2_dx:k_conv_dx_lds", "conv3_dx:k_conv_dx_lds"};
    const dim3 block(p.block);
    switch (p.kernel) {
      case CONV_DX_T16_MULTI:
        if constexpr (dx_t16_geom(G::KS, G::S, G::IH)) { RB_LAUNCH_T(tags[layer], (k_conv_dx_t16_multi<G, 64, lazy>), p.grid, block, stream, a); }
        break;
      case CONV_DX_LDS_MULTI:
        if constexpr (!dx_t16_geom(G::KS, G::S, G::IH)) { RB_LAUNCH_T(tags[layer], (k_conv_dx_lds<G, NT, 64, lazy, true>), p.grid, block, stream, a); }
        break;
      case CONV_DX_LDS:
        RB_LAUNCH_T(tags[layer], (k_conv_dx_lds<G, NT, 64, lazy, false>), p.grid, block, stream, a);
        break;
      default: break;
    }
    RB_LAUNCH_CHECK();
  }
  return RB_OK;
}
static int conv_dx(rb_learner* l, int layer, hipStream_t stream) {
  return with_geom(l->L.conv[layer], [&](auto cfg) { return launch_conv_dx<decltype(cfg)>(l, layer, stream); });
}

// the weight / bias gradient of ONE layer on the gemm_core.h fallback (split slices, summed by k_reduce_conv_dw_all after the last layer)
template <class C>
static int launch_conv_dw_gemm(rb_learner* l, int layer, const uint8_t* states, hipStream_t stream) {
  using G = typename C::G;
  const Layout& L = l->L;
  const ConvLayer& c = L.conv[layer];
  const ConvDwGemmPlan p = plan_conv_dw_gemm(plan_in(l), layer);
  if (layer == 0) {
    ConvDwProb<G, true> q;
    q.B = L.B; q.cin = c.cin; q.cout = c.cout; q.splits = p.splits;
    q.dy = l->dact[0]; q.x_u8 = states; q.x_f = nullptr; q.part = l->dw_part[0];
    RB_LAUNCH((k_gemm<1, 2, ConvDwProb<G, true>>), p.grid, dim3(p.block), stream, q);
  } else {
    ConvDwProb<G, false> q;
    q.B = L.B; q.cin = c.cin; q.cout = c.cout; q.splits = p.splits;
    q.dy = l->dact[layer]; q.x_u8 = nullptr; q.x_f = l->act[layer - 1]; q.part = l->dw_part[layer];
    RB_LAUNCH((k_gemm<2, 2, ConvDwProb<G, false>>), p.grid, dim3(p.block), stream, q);
  }
  RB_LAUNCH_CHECK();
  l->dw_slices[layer] = p.splits;
  return RB_OK;
}
static int conv_dw_gemm(rb_learner* l, int layer, const uint8_t* states, hipStream_t stream) {
  return with_geom(l->L.conv[layer], [&](auto cfg) { return launch_conv_dw_gemm<decltype(cfg)>(l, layer, states, stream); });
}

// all conv layers' weight gradients in one launch (LDS kernels); fills dw_slices for the fused slice reduction
static int conv_dw_all(rb_learner* l, hipStream_t stream) {
  const Layout& L = l->L;
  const ConvDwAllPlan p = plan_conv_dw_all(plan_in(l));
  ConvDwAllArgs a;
  a.batch = L.B;
  a.img_fast = p.img_fast;
  for (int i = 0; i < 3; ++i) { a.ipb[i] = p.ipb[i]; a.cotiles[i] = p.cotiles[i]; a.nblocks[i] = p.nblocks[i]; }
  for (int i = 0; i < L.nconv; ++i) {
    const ConvLayer& c = L.conv[i];
    ConvLdsDwArgs& d = a.layer[i];
    d.cin = c.cin; d.cout = c.cout; d.dy = l->dact[i]; d.part = l->dw_part[i];
    d.src = l->cur_src; d.x_f = i > 0 ? l->act[i - 1] : nullptr;
    d.dy_part = l->dfeat_part; d.dy_mask = l->act[i]; d.dy_stride = (int64_t)L.B * L.F;
    d.dy_splits = (l->lazy_dfeat && i == L.nconv - 1 && i > 0) ? l->lazy_splits : 0;
    l->dw_slices[i] = p.dw_slices[i];
  }
  for (int i = L.nconv; i < 3; ++i) a.layer[i] = a.layer[0];
  // (a pipelined body — two operand sets in LDS, the next image's loads in flight under this image's MFMAs — was built in round 5,
  // bit-identical, and measured SLOWER at batch 256: 75.9 against 64.5 us for this launch, profiles/round5_experiments.txt; removed)
  if (L.nconv == 3) {
    RB_LAUNCH_T("conv_dw_all", (k_conv_dw_all<GeomC1, 7, GeomC2, 9, 512, GeomC3, 7, 576, 3>), dim3(p.total), dim3(RB_CONV_THREADS), stream, a);
  } else {
    RB_LAUNCH_T("conv_dw_all", (k_conv_dw_all<GeomD1, 4, GeomD2, 3, 800, GeomD2, 3, 800, 2>), dim3(p.total), dim3(RB_CONV_THREADS), stream, a);
  }
  RB_LAUNCH_CHECK();
  return RB_OK;
}
