// The nonconformity score of the conformal kernels (include/tecmollm.h (3g)), shared by conformal_scores_kernel and
// interval_stats_kernel (conformal.hip) so that calibration and scoring see the same bits of every score: a score stored by
// (a) and the score (c) compares with a quantile selected from that store are the result of the same instructions.
#pragma once
#include "common.h"
#include "metrics_value.h"

// raw scaled prediction and truth -> float32 p, y in physical units (the value pipeline of metrics_map_kernel)
static __device__ __forceinline__ void conformal_values(float praw, float yraw, double mean, double scale, int clip,
                                                        float clip_lo, float clip_hi, float& p, float& y) {
  if (!isfinite(praw)) praw = 0.f;
  p = nan_to_num_tec(unscale_f32(praw, mean, scale));
  y = nan_to_num_tec(unscale_f32(yraw, mean, scale));
  if (clip) p = fminf(fmaxf(p, clip_lo), clip_hi);
}
// w = max(sigma, sigma_min); fmaxf returns the other operand for a NaN, so a NaN sigma counts as sigma_min
static __device__ __forceinline__ float conformal_weight(float sigma, float sigma_min) { return fmaxf(sigma, sigma_min); }
// one f32 subtraction, and with a scale one IEEE f32 division (this library is built without fast-math)
static __device__ __forceinline__ float conformal_score(float p, float y, int mode, bool scaled, float w) {
  float r = y - p;
  if (mode == TECM_CONF_ABS) r = fabsf(r);
  if (scaled) r = r / w;
  return r;
}
