// The value pipeline of the evaluation statistics (src/evaluation/metrics.py:36-51), shared by metrics_kernel
// (trainstep.hip) and metrics_map_kernel (metrics_map.hip) so that both see the same bits of every (t, p) pair.
#pragma once
#include "common.h"

static __device__ __forceinline__ float unscale_f32(float y, double mean, double scale) {
  // sklearn StandardScaler.inverse_transform on a float32 array: X *= scale_ ; X += mean_ (two f32 roundings)
  const float a = (float)((double)y * scale);
  return (float)((double)a + mean);
}
static __device__ __forceinline__ float nan_to_num_tec(float v) {
  if (v != v) return 0.f;
  if (isinf(v)) return v > 0.f ? 100.f : 0.f;
  return v;
}
