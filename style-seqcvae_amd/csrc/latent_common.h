// The two expressions every reader of the latent head shares (pointwise.hip: the train step's forward, backward and prior sample;
// score.hip: the posterior rows).  Device inline code only.
#pragma once
#include "ssc_common.h"

// The prior mean of element (row, z): a per-element one (pm, leading dimension ldpm: the attention-pooled attribute means) wins over
// the per-row one (pm_scale * sent[row]); neither: 0.
__device__ __forceinline__ float latent_prior_mean(const float* pm, int ldpm, const float* sent, float pm_scale, size_t row, int z) {
  return pm ? pm[row * ldpm + z] : (sent ? pm_scale * sent[row] : 0.f);
}

// k_tbj, the training KL of one element (var = exp(l); lpv = log(pvar)).  The forward's sums, the mode-1 gates of the free-bits
// backward and the posterior rows all form it HERE: one expression, one order.
__device__ __forceinline__ float latent_kl_elem(int kld_mode, float m, float l, float var, float pm, float lpv, float pvar) {
  if (kld_mode == 0) return -0.5f * (1.f + l - m * m - var);
  const float dm = m - pm;
  return -0.5f * (1.f + l - lpv - (dm * dm + var) / (pvar + 0.00001f));
}
