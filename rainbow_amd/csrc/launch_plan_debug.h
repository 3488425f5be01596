// launch_plan_debug.h — rb_debug_launch_plan: the plans of learner_plan.h as text, one line per launch of a learn step, in launch
// order (the sequence of learn_impl), then the forward lines of a one-row f32 forward and the act path's row groups.  Stateless: no handle, no device.
// Included by learner.hip only.
#pragma once
#include "learner_plan.h"

struct PlanText {
  char* out;
  int64_t cap, len;
  bool full;
  void line(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const int64_t room = cap - len;
    const int n = room > 0 ? vsnprintf(out + len, (size_t)room, fmt, ap) : 0;
    va_end(ap);
    if (room <= 0 || n < 0 || n + 1 >= room) { full = true; return; }
    len += n;
    out[len++] = '\n';
    out[len] = 0;
  }
};

static void plan_text_forward(PlanText& t, const PlanIn& in, const char* prefix, int n_on, int n_tg, bool f32) {
  const Layout& L = in.L;
  for (int layer = 0; layer < L.nconv; ++layer) {
    const ConvFwdPlan p = plan_conv_fwd(in, layer, n_on, n_tg, f32);
    char name[96];
    if (p.kernel == CONV_FWD_GEMM) snprintf(name, sizeof(name), "k_gemm<ConvFwdProb<%s>>", p.geom);
    else snprintf(name, sizeof(name), "%s<%s%s>", conv_fwd_kernel_name[p.kernel], p.geom, p.kernel == CONV_FWD_LDS_F32 ? ",F32SRC" : "");
    t.line("%sconv%d_fwd kernel=%s grid=%ux%ux%u block=%u ipb=%d img_fast=%d", prefix, layer + 1, name, p.grid.x, p.grid.y, p.grid.z,
           p.block, p.ipb, p.img_fast);
  }
  const FcFwdPlan f = plan_fc_fwd(in, n_on, n_tg);
  if (f.block_copy) t.line("%sfeat_block_copy kernel=k_block_copy", prefix);
  t.line("%sfc_h_fwd kernel=%s grid=%ux%ux%u block=%u tiles=%d S=%d", prefix, fc_fwd_kernel_name[f.h_kernel], f.hgrid.x, f.hgrid.y,
         f.hgrid.z, f.hblock, f.tiles, f.S);
  if (f.h_kernel == FC_FWD_KGEMM) t.line("%sfc_h_finish kernel=k_fc_h_finish splits=%d", prefix, in.caps.hs);
  t.line("%sfc_z_fwd kernel=%s grid=%ux%ux%u block=%u", prefix, fc_fwd_kernel_name[f.z_kernel], f.zgrid.x, f.zgrid.y, f.zgrid.z, f.zblock);
}

extern "C" int rb_debug_launch_plan(const rb_learner_config_t* cfg, const char* rb_opts, int32_t n_cu, int32_t flags, int32_t world,
                                    int32_t with_sink, char* out, int64_t cap) {
  RB_REQUIRE(out != nullptr && cap >= 1, "rb_debug_launch_plan: no output buffer");
  RB_REQUIRE(n_cu >= 1 && world >= 1, "rb_debug_launch_plan: n_cu and world must be >= 1");
  Layout L;
  int rc = make_layout(cfg, &L);
  if (rc != RB_OK) return rc;
  RbOpts opt;
  rc = rb_opts_parse(rb_opts, &opt);
  if (rc != RB_OK) return rc;
  const LearnerCaps caps = plan_caps(L, opt);
  const PlanIn in{L, opt, caps, n_cu, flags, world > 1 && caps.fast_fc, with_sink != 0};
  PlanText t{out, cap, 0, false};
  out[0] = 0;
  t.line("caps fast_fc=%d fast_conv=%d hs=%d xs=%d ws=%d/%d/%d wT=%d/%d/%d gemm_ws=%d", caps.fast_fc, caps.fast_conv, caps.hs, caps.xs,
         caps.ws[0], caps.ws[1], caps.ws[2], caps.wT[0], caps.wT[1], caps.wT[2], caps.gemm_ws);
  plan_text_forward(t, in, "", 2 * L.B, L.B, false);
  {
    const HeadPlan h = plan_head(in);
    t.line("head kernel=k_head<%d> grid=%ux1x1 block=%d samples=%d tenants=%d waves=%d wt_t16=%d/%d", h.ZI, h.blocks, 64 * h.waves, L.B,
           h.n_jobs > 0 ? 2 * h.per_job : 0, h.waves, h.job_t16[0], h.job_t16[1]);
  }
  const FcBwdPlan b = plan_fc_bwd(in, false);
  if (b.z_kernel == FC_BWD_KGEMM) {
    t.line("fc_z_dw kernel=k_gemm<FcZDwProb> grid=%ux%ux%u block=128", b.gz_dw.x, b.gz_dw.y, b.gz_dw.z);
    t.line("fc_z_dx kernel=k_gemm<FcZDxProb> grid=%ux%ux%u block=64", b.gz_dx.x, b.gz_dx.y, b.gz_dx.z);
    t.line("fc_h_dw kernel=k_gemm<FcHDwProb> grid=%ux%ux%u block=256", b.gh_dw.x, b.gh_dw.y, b.gh_dw.z);
    t.line("fc_h_dx kernel=k_gemm<FcHDxProb> grid=%ux%ux%u block=128", b.gh_dx.x, b.gh_dx.y, b.gh_dx.z);
    t.line("dfeat_finish kernel=k_dfeat_finish splits=%d", b.hsplits);
  } else {
    t.line("fc_z_bwd kernel=%s grid=%ux1x1 block=%u dw=%dx%d dx=%dx%dx%d pipe=%d z_ct=%d z_tall=%d", fc_bwd_kernel_name[b.z_kernel], b.z_blocks,
           b.z_threads, b.zg.dw_x, b.zg.dw_y, b.zg.dx_x, b.zg.dx_y, b.zg.dx_z, b.pipe ? 1 : 0, b.z_ct, b.z_tall ? 1 : 0);
    if (b.pack) t.line("pack_factors kernel=k_pack_factors grid=16x5x1 block=256");
    t.line("fc_h_bwd kernel=%s grid=%ux1x1 block=%u dw=%dx%d dx=%dx%dx%d writeback=%d h_ct=%d gemm_bwd=%d fuse_norm=%d defer_dw=%d "
           "implicit_sigma=%d hsplits=%d rows_per_split=%d norm_slots=%d lazy_dfeat=%d", fc_bwd_kernel_name[b.h_kernel], b.h_blocks, b.h_threads, b.hg.dw_x, b.hg.dw_y,
           b.hg.dx_x, b.hg.dx_y, b.hg.dx_z, b.up_enabled ? 1 : 0, b.h_ct, b.gemm_bwd ? 1 : 0, b.fuse_norm ? 1 : 0, b.defer_dw ? 1 : 0,
           b.implicit_sigma ? 1 : 0, b.hsplits, b.rows_per_split, b.norm_slots, b.lazy_dfeat ? 1 : 0);
    if (!b.lazy_dfeat) t.line("dfeat_finish kernel=k_dfeat_finish splits=%d", b.hsplits);
  }
  auto dx_line = [&](int layer) {
    const ConvDxPlan p = plan_conv_dx(in, layer, b.lazy_dfeat);
    if (p.kernel == CONV_DX_NONE) return;
    char name[96];
    if (p.kernel == CONV_DX_GEMM) snprintf(name, sizeof(name), "k_gemm<ConvDxProb<%s>>", p.geom);
    else if (p.kernel == CONV_DX_T16_MULTI) snprintf(name, sizeof(name), "k_conv_dx_t16_multi<%s>", p.geom);
    else snprintf(name, sizeof(name), "k_conv_dx_lds<%s,MULTI=%s>", p.geom, p.kernel == CONV_DX_LDS_MULTI ? "true" : "false");
    t.line("conv%d_dx kernel=%s grid=%ux%ux%u block=%u ipb=%d img_fast=%d wt_t16=%d", layer + 1, name, p.grid.x, p.grid.y, p.grid.z, p.block,
           p.ipb, p.img_fast, p.wt_t16);
  };
  if (caps.fast_conv) {
    for (int layer = L.nconv - 1; layer > 0; --layer) dx_line(layer);
    const ConvDwAllPlan d = plan_conv_dw_all(in);
    t.line("conv_dw_all kernel=k_conv_dw_all<%d> grid=%ux1x1 block=%d ipb=%d/%d/%d nblocks=%d/%d/%d slices=%d/%d/%d img_fast=%d", L.nconv, d.total,
           RB_CONV_THREADS, d.ipb[0], d.ipb[1], d.ipb[2], d.nblocks[0], d.nblocks[1], d.nblocks[2], d.dw_slices[0], d.dw_slices[1],
           d.dw_slices[2], d.img_fast);
  } else {
    for (int layer = L.nconv - 1; layer >= 0; --layer) {
      const ConvDwGemmPlan d = plan_conv_dw_gemm(in, layer);
      t.line("conv%d_dw kernel=k_gemm<ConvDwProb> grid=%ux%ux%u block=%u splits=%d", layer + 1, d.grid.x, d.grid.y, d.grid.z, d.block, d.splits);
      dx_line(layer);
    }
  }
  t.line("reduce_conv_dw kernel=k_reduce_conv_dw_all grid=%ux1x1 block=64 snapshot=%d", plan_conv_reduce_blocks(L, b.implicit_sigma),
         b.implicit_sigma ? 1 : 0);
  plan_text_forward(t, in, "act_", 1, 0, true);
  {
    // rb_learner_act's own path (act_host.h): covered=0 is the training forward above; rg = output rows per workgroup and layer
    int rg[3];
    const bool covered = act_path_covers(L, caps, rg);
    t.line("act_path covered=%d rg=%d/%d/%d", covered ? 1 : 0, rg[0], rg[1], rg[2]);
  }
  if (t.full) {
    rb_set_error("rb_debug_launch_plan: %lld bytes are too few for the plan", (long long)cap);
    return RB_ERR_INVALID;
  }
  return RB_OK;
}
