// exchange_host.h — the replica exchange: the factor all-gather and the launch that finishes the gradients from the
// gathered rows.  Included by learner.hip only, after grad_finish.h (k_finish_grads*) and fc_dispatch.h (fc_dw_plan).
#pragma once
#include "learner_plan.h"

extern "C" {

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
  int c_slots = plan_sumsq_blocks(conv_n);
  for (FcDwPlan* p : {&zp, &hp}) {
    p->a.rpb = L.B; p->a.bstride = l->fact_stride; p->a.scale = 1.0f / (float)l->world;
    p->a.noise_blocks = f + l->fact_off[4];
  }
  zp.a.eout_noff = L.z_eout; zp.a.ein_noff = L.z_ein;
  hp.a.eout_noff = L.h_eout; hp.a.ein_noff = L.h_ein;
  // the hidden layer on 128 x 128 LDS tiles (fc_gemm.h rb_fc_gemm_dw_ranks): a rank's slab of the gathered factors is read once
  // per 128 weight rows instead of once per 16 (narrower layers: the 16-row-tile body)
  const bool tiled = 2 * L.H >= 64 && L.F >= 64;
  const int h_nt = (int)rb_div_up(2 * L.H, RB_TG_T), h_kt = (int)rb_div_up(L.F, RB_TG_T);
  if (tiled) {
    // (every workgroup of this launch is 512 threads at ~250 registers: ONE per CU.  The output layer's tiles therefore take all
    // eight waves — 512 columns per workgroup, 23 instead of 46 workgroups at the canonical shape — so that the launch stays within
    // one round of 256: with 266 workgroups the last ten waited for a CU and the launch took 40 us instead of 27)
    hp.slots = 8 * h_nt * h_kt;
    zp.dw_x = (int)rb_div_up(zp.a.K, 512);
    zp.slots = 8 * zp.dw_x * zp.dw_y;
    c_slots = h_nt * h_kt;         // the conv range: one slice (and one partial) per tile workgroup
  }
  RB_REQUIRE(zp.slots + hp.slots + c_slots <= 16384, "rb_learner_finish_grads: too many norm partials");
  FinishArgs fa;
  if (tiled) { hp.a.sq_part = l->norm_part; zp.a.sq_part = l->norm_part + hp.slots; }
  else { zp.a.sq_part = l->norm_part; hp.a.sq_part = l->norm_part + zp.slots; }
  fa.z = zp.a; fa.h = hp.a;
  fa.z_x = zp.dw_x; fa.z_n = zp.dw_x * zp.dw_y; fa.h_x = hp.dw_x; fa.h_n = hp.dw_x * hp.dw_y;
  // the conv gradients travel in the same blocks: their replica mean (rank order) and its sum of squares (0.3 MB per rank);
  // tiled: sliced over the hidden layer's tile workgroups (c_slots above)
  fa.g = l->grads; fa.n = conv_n; fa.part = l->norm_part + zp.slots + hp.slots; fa.nparts = c_slots;
  fa.blocks = f + l->fact_off[5]; fa.bstride = l->fact_stride; fa.world = l->world; fa.scale = 1.0f / (float)l->world;
  if (tiled) {
    RB_LAUNCH_T("finish_grads:k_finish_grads", k_finish_grads_tiled, dim3((unsigned)(h_nt * h_kt + fa.z_n)), dim3(RB_TG_THREADS), stream, fa, h_nt, h_kt);
  } else {
    RB_LAUNCH_T("finish_grads:k_finish_grads", k_finish_grads, dim3((unsigned)(fa.z_n + fa.h_n + c_slots)), dim3(256), stream, fa);
  }
  RB_LAUNCH_CHECK();
  l->norm_slots = zp.slots + hp.slots + c_slots;
  l->exch_pending = 0;
  return RB_OK;
}

}  // extern "C"
