// What the LayerNorm kernels (layernorm.hip) and the column sums (colsum.hip) share: the dropout context a kernel carries
// for a mask it applies or undoes on the way.
#pragma once
#include "common.h"

namespace {

struct DropCtxN {
  uint64_t seed;
  int64_t ld;
  uint32_t thresh;
  float inv;
  const uint64_t* sdev;        // TecmDrop::seed_dev: added to seed when the kernel starts (seed_now below)
};
__device__ __forceinline__ void seed_now(DropCtxN& c) { c.seed = tecm_seed_now(c.seed, c.sdev); }
__host__ __device__ inline DropCtxN make_dropn(const TecmDrop* d) {
  DropCtxN c;
  c.seed = d ? d->seed : 0;
  c.sdev = d ? d->seed_dev : nullptr;
  c.ld = d ? d->ld : 0;
  c.thresh = (d && d->p > 0.f) ? tecm_drop_thresh(d->p) : 0u;
  c.inv = (d && d->p > 0.f) ? 1.0f / (1.0f - d->p) : 1.0f;
  return c;
}

}  // namespace
