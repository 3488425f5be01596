// exchange_host.h — the replica exchange: the factor all-gather and the launch that finishes the gradients from the
// gathered rows.  Included by learner.hip only, after grad_finish.h (k_finish_grads_tiled) and fc_dispatch.h (fc_dw_plan).
#pragma once
#include "learner_plan.h"

// The tiles of rb_learner_finish_grads' one launch and the sum-of-squares slots they write — a function of the layout alone, so
// rb_learner_set_exchange can refuse a layout whose slots do not fit before any learn call runs.  The hidden layer goes on 128 x 128
// LDS tiles (fc_gemm.h rb_fc_gemm_dw_ranks): a rank's slab of the gathered factors is read once per 128 weight rows instead of
// once per 16.  (fast_fc, which the exchange requires, means H % 32 == 0 and F = 3136 or 576: 2H >= 64 and F >= 64 always hold, so
// there is no narrower form.)
// (every workgroup of the launch is 512 threads at ~250 registers: ONE per CU.  The output layer's tiles therefore take all
// eight waves — 512 columns per workgroup, 23 instead of 46 workgroups at the canonical shape — so that the launch stays within
// one round of 256: with 266 workgroups the last ten waited for a CU and the launch took 40 us instead of 27)
struct FinishPlan {
  int h_nt, h_kt;           // hidden layer: 128-row x 128-column tiles, 8 slots (waves) each
  int z_x, z_y;             // output layer: 512-column workgroups x 16-row tiles, 8 slots each
  int h_slots, z_slots, c_slots;      // c_slots: the conv range, one slice (and one partial) per hidden-layer tile workgroup
  int slots() const { return h_slots + z_slots + c_slots; }
};
static FinishPlan plan_finish(const Layout& L) {
  FinishPlan p;
  p.h_nt = (int)rb_div_up(2 * L.H, RB_TG_T); p.h_kt = (int)rb_div_up(L.F, RB_TG_T);
  p.z_x = (int)rb_div_up(L.H, 512); p.z_y = plan_fc_dw_tiles(L, 0, 0).dw_y;
  p.h_slots = 8 * p.h_nt * p.h_kt;
  p.z_slots = 8 * p.z_x * p.z_y;
  p.c_slots = p.h_nt * p.h_kt;
  return p;
}

extern "C" {

// One rank's block, six segments, each rounded up to 64 floats (the gaps are never read):
//   dlogits [B][NZ] | h [B][2H] | dh [B][2H] | feat [B][F] | noise [n_noise] | conv grads [small_floats]
// factor_floats is their total (the stride between two ranks' blocks in the gathered buffer); the conv gradients are the leading
// small_floats of the flat gradient buffer (small_offset = 0).
int rb_learner_exchange_layout(rb_learner_t* l, int64_t* factor_floats, int64_t* small_offset, int64_t* small_floats) {
  RB_REQUIRE(l != nullptr, "rb_learner_exchange_layout: NULL handle");
  if (factor_floats) *factor_floats = l->fact_stride;
  if (small_offset) *small_offset = 0;            // the conv parameters lead the flat buffers (make_layout)
  if (small_floats) *small_floats = l->L.h_mu;
  return RB_OK;
}

int rb_learner_set_exchange(rb_learner_t* l, int32_t world, float* factors_local_dev, const float* factors_all_dev) {
  RB_REQUIRE(l != nullptr, "rb_learner_set_exchange: NULL handle");
  RB_REQUIRE(world >= 1 && world <= 64, "rb_learner_set_exchange: world must be in [1,64]");
  if (world == 1) { l->world = 1; l->fact_local = nullptr; l->fact_all = nullptr; return RB_OK; }
  RB_REQUIRE(factors_local_dev && factors_all_dev, "rb_learner_set_exchange: NULL factor buffer");
  if (!l->caps.fast_fc) {
    rb_set_error("rb_learner_set_exchange: the factored exchange needs the streamed noisy-linear kernels (F, H multiples of 32); "
                 "all-reduce the flat gradient and call rb_learner_grads_modified instead");
    return RB_ERR_STATE;
  }
  const FinishPlan fp = plan_finish(l->L);
  if (fp.slots() > RB_NORM_PART_SLOTS) {
    rb_set_error("rb_learner_set_exchange: rb_learner_finish_grads would need %d sum-of-squares slots at this shape, %d exist; "
                 "all-reduce the flat gradient and call rb_learner_grads_modified instead", fp.slots(), RB_NORM_PART_SLOTS);
    return RB_ERR_STATE;
  }
  l->world = world; l->fact_local = factors_local_dev; l->fact_all = factors_all_dev;
  return RB_OK;
}

int rb_learner_wait_factors(rb_learner_t* l, rb_stream_t side_stream) {
  RB_REQUIRE(l != nullptr, "rb_learner_wait_factors: NULL handle");
  RB_REQUIRE(l->exch_pending, "rb_learner_wait_factors: no learn call with a pending exchange");
  (void)side_stream;     // the block is complete in the stream order of the learn call: nothing to wait for (see the header)
  return RB_OK;
}

int rb_learner_exchange_rccl(rb_learner_t* l, rb_comm_t* comm, rb_stream_t stream_) {
  RB_REQUIRE(l && comm, "rb_learner_exchange_rccl: NULL argument");
  RB_REQUIRE(l->exch_pending && l->fact_local && l->fact_all, "rb_learner_exchange_rccl: no learn call with a pending exchange");
  const int cw = rb_comm_world(comm);
  RB_REQUIRE(cw == l->world || (cw == 1 && l->world == 2),
             "rb_learner_exchange_rccl: the communicator has %d ranks, the exchange buffer %d blocks", cw, l->world);
  hipStream_t stream = (hipStream_t)stream_;
  float* all = const_cast<float*>(l->fact_all);
  const int rc = rb_comm_all_gather_f32(comm, l->fact_local, all, (size_t)l->fact_stride, stream);
  if (rc != RB_OK) return rc;
  if (cw == 1 && l->world == 2)      // single-GPU plumbing run: the lone block stands for both replicas
    RB_HIP_TRY(hipMemcpyAsync(all + l->fact_stride, all, (size_t)l->fact_stride * 4, hipMemcpyDeviceToDevice, stream));
  return rb_learner_finish_grads(l, stream_);
}

int rb_learner_finish_grads(rb_learner_t* l, rb_stream_t stream_) {
  RB_REQUIRE(l != nullptr, "rb_learner_finish_grads: NULL handle");
  RB_REQUIRE(l->exch_pending, "rb_learner_finish_grads: no learn call with a pending exchange");
  RB_FLUSH_UPDATE(l, stream_);
  hipStream_t stream = (hipStream_t)stream_;
  const Layout& L = l->L;
  const NetPtrs on = net_ptrs(L, l->p_online, l->n_online);
  const int M = l->world * L.B;
  const float* f = l->fact_all;
  FcDwPlan zp = fc_dw_plan(l, on, 0, f + l->fact_off[0], f + l->fact_off[1], M, 0);
  FcDwPlan hp = fc_dw_plan(l, on, 1, f + l->fact_off[2], f + l->fact_off[3], M, 0);
  const int64_t conv_n = L.h_mu;
  for (FcDwPlan* p : {&zp, &hp}) {
    p->a.rpb = L.B; p->a.bstride = l->fact_stride; p->a.scale = 1.0f / (float)l->world;
    p->a.noise_blocks = f + l->fact_off[4];
  }
  zp.a.eout_noff = L.z_eout; zp.a.ein_noff = L.z_ein;
  hp.a.eout_noff = L.h_eout; hp.a.ein_noff = L.h_ein;
  const FinishPlan fp = plan_finish(L);
  hp.slots = fp.h_slots;
  zp.dw_x = fp.z_x;
  zp.slots = fp.z_slots;
  const int c_slots = fp.c_slots;
  // (rb_learner_set_exchange has refused such a layout already: a backstop)
  RB_REQUIRE(fp.slots() <= RB_NORM_PART_SLOTS, "rb_learner_finish_grads: too many norm partials");
  FinishArgs fa;
  hp.a.sq_part = l->norm_part; zp.a.sq_part = l->norm_part + hp.slots;
  fa.z = zp.a; fa.h = hp.a;
  fa.z_x = zp.dw_x; fa.z_n = zp.dw_x * zp.dw_y;
  // the conv gradients travel in the same blocks: their replica mean (rank order) and its sum of squares (0.3 MB per rank),
  // sliced over the hidden layer's tile workgroups (c_slots)
  fa.g = l->grads; fa.n = conv_n; fa.part = l->norm_part + zp.slots + hp.slots; fa.nparts = c_slots;
  fa.blocks = f + l->fact_off[5]; fa.bstride = l->fact_stride; fa.world = l->world; fa.scale = 1.0f / (float)l->world;
  RB_LAUNCH_T("finish_grads:k_finish_grads", k_finish_grads_tiled, dim3((unsigned)(fp.h_nt * fp.h_kt + fa.z_n)), dim3(RB_TG_THREADS), stream, fa,
              fp.h_nt, fp.h_kt);
  RB_LAUNCH_CHECK();
  l->norm_slots = zp.slots + hp.slots + c_slots;
  l->exch_pending = 0;
  return RB_OK;
}

}  // extern "C"
