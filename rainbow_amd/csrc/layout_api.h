// layout_api.h — the layout and descriptor entry points (no device, no handle).  Included by learner.hip only.
#pragma once
#include "learner_internal.h"

extern "C" {

int rb_learner_sizes(const rb_learner_config_t* cfg, int64_t* n_params, int64_t* n_noise) {
  Layout L;
  int rc = make_layout(cfg, &L);
  if (rc != RB_OK) return rc;
  if (n_params) *n_params = L.n_params;
  if (n_noise) *n_noise = L.n_noise;
  return RB_OK;
}

static void set_desc(rb_tensor_desc_t* d, const char* name, int64_t off, int ndim, int s0, int s1, int s2, int s3) {
  memset(d, 0, sizeof(*d));
  snprintf(d->name, sizeof(d->name), "%s", name);
  d->offset = off; d->ndim = ndim;
  d->shape[0] = s0; d->shape[1] = s1; d->shape[2] = s2; d->shape[3] = s3;
}

int rb_learner_param_layout(const rb_learner_config_t* cfg, rb_tensor_desc_t* descs, int32_t* n) {
  Layout L;
  int rc = make_layout(cfg, &L);
  if (rc != RB_OK) return rc;
  RB_REQUIRE(n != nullptr, "rb_learner_param_layout: n is NULL");
  const int count = 2 * L.nconv + 16;
  if (!descs) { *n = count; return RB_OK; }
  RB_REQUIRE(*n >= count, "rb_learner_param_layout: need room for %d descriptors", count);
  int i = 0;
  char name[48];
  for (int l = 0; l < L.nconv; ++l) {
    const ConvLayer& c = L.conv[l];
    snprintf(name, sizeof(name), "convs.%d.weight", 2 * l);
    set_desc(&descs[i++], name, L.conv_w[l], 4, c.cout, c.cin, c.ks, c.ks);
    snprintf(name, sizeof(name), "convs.%d.bias", 2 * l);
    set_desc(&descs[i++], name, L.conv_b[l], 1, c.cout, 0, 0, 0);
  }
  const int64_t HF = (int64_t)L.H * L.F, ZH = (int64_t)L.Z * L.H;
  const int AZ = L.A * L.Z;
  set_desc(&descs[i++], "fc_h_v.weight_mu", L.h_mu, 2, L.H, L.F, 0, 0);
  set_desc(&descs[i++], "fc_h_v.weight_sigma", L.h_sigma, 2, L.H, L.F, 0, 0);
  set_desc(&descs[i++], "fc_h_v.bias_mu", L.h_bmu, 1, L.H, 0, 0, 0);
  set_desc(&descs[i++], "fc_h_v.bias_sigma", L.h_bsigma, 1, L.H, 0, 0, 0);
  set_desc(&descs[i++], "fc_h_a.weight_mu", L.h_mu + HF, 2, L.H, L.F, 0, 0);
  set_desc(&descs[i++], "fc_h_a.weight_sigma", L.h_sigma + HF, 2, L.H, L.F, 0, 0);
  set_desc(&descs[i++], "fc_h_a.bias_mu", L.h_bmu + L.H, 1, L.H, 0, 0, 0);
  set_desc(&descs[i++], "fc_h_a.bias_sigma", L.h_bsigma + L.H, 1, L.H, 0, 0, 0);
  set_desc(&descs[i++], "fc_z_v.weight_mu", L.z_mu, 2, L.Z, L.H, 0, 0);
  set_desc(&descs[i++], "fc_z_v.weight_sigma", L.z_sigma, 2, L.Z, L.H, 0, 0);
  set_desc(&descs[i++], "fc_z_v.bias_mu", L.z_bmu, 1, L.Z, 0, 0, 0);
  set_desc(&descs[i++], "fc_z_v.bias_sigma", L.z_bsigma, 1, L.Z, 0, 0, 0);
  set_desc(&descs[i++], "fc_z_a.weight_mu", L.z_mu + ZH, 2, AZ, L.H, 0, 0);
  set_desc(&descs[i++], "fc_z_a.weight_sigma", L.z_sigma + ZH, 2, AZ, L.H, 0, 0);
  set_desc(&descs[i++], "fc_z_a.bias_mu", L.z_bmu + L.Z, 1, AZ, 0, 0, 0);
  set_desc(&descs[i++], "fc_z_a.bias_sigma", L.z_bsigma + L.Z, 1, AZ, 0, 0, 0);
  *n = i;
  return RB_OK;
}

int rb_learner_noise_layout(const rb_learner_config_t* cfg, rb_tensor_desc_t* descs, int32_t* n) {
  Layout L;
  int rc = make_layout(cfg, &L);
  if (rc != RB_OK) return rc;
  RB_REQUIRE(n != nullptr, "rb_learner_noise_layout: n is NULL");
  if (!descs) { *n = 8; return RB_OK; }
  RB_REQUIRE(*n >= 8, "rb_learner_noise_layout: need room for 8 descriptors");
  int i = 0;
  set_desc(&descs[i++], "fc_h_v.eps_in", L.h_ein, 1, L.F, 0, 0, 0);
  set_desc(&descs[i++], "fc_h_v.eps_out", L.h_eout, 1, L.H, 0, 0, 0);
  set_desc(&descs[i++], "fc_h_a.eps_in", L.h_ein + L.F, 1, L.F, 0, 0, 0);
  set_desc(&descs[i++], "fc_h_a.eps_out", L.h_eout + L.H, 1, L.H, 0, 0, 0);
  set_desc(&descs[i++], "fc_z_v.eps_in", L.z_ein, 1, L.H, 0, 0, 0);
  set_desc(&descs[i++], "fc_z_v.eps_out", L.z_eout, 1, L.Z, 0, 0, 0);
  set_desc(&descs[i++], "fc_z_a.eps_in", L.z_ein + L.H, 1, L.H, 0, 0, 0);
  set_desc(&descs[i++], "fc_z_a.eps_out", L.z_eout + L.Z, 1, L.A * L.Z, 0, 0, 0);
  *n = i;
  return RB_OK;
}

int64_t rb_learner_noise_draws(const rb_learner_config_t* cfg) {
  Layout L;
  if (make_layout(cfg, &L) != RB_OK) return -1;
  return 2 * (int64_t)L.F + 2 * (int64_t)L.H + 2 * (int64_t)L.H + L.NZ;
}

}  // extern "C"
