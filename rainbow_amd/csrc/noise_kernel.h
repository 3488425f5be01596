// noise_kernel.h — the factorised-noise generator as a launch of its own (noise_body.h has the body the sampler launch hosts).
// Included by learner.hip only.
#pragma once
#include "noise_body.h"

// ------------------------------------------------------------------------ noise --
// f(x) = sign(x) * sqrt(|x|)  (model.py:32-34).  raw == NULL: N(0,1) from Philox + Box-Muller.
// Draw order = the reference's: per layer randn(in) then randn(out); fc_h_v, fc_h_a, fc_z_v,
// fc_z_a (model.py:36-38, 82-85).
__global__ __launch_bounds__(256) void k_noise(float* noise, float* noise2, const float* raw, NoiseMap map, uint64_t seed,
                                                unsigned long long* ctr) {
  rb_noise_body(noise, noise2, raw, map, seed, ctr, (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.y, (int)gridDim.y);
}
