// The GATv2 edge math of the fused spatial stage, once, for every kernel of the family (spatial_fwd.hip, spatial_fwd2.hip,
// spatial_bwd.hip, spatial_bwd2.hip, spatial_dx.hip, spatial_attn.hip): head-sliced row loads and stores, the logit in its
// three forms, the online-softmax steps, what `de` adds to d x_r / d att / d x_l and the index of the alpha-dropout mask
// (the decode of a graph number is in spatial_common.h).  With
//     e_ij = att . lrelu(x_l[j] + x_r[i])      alpha = softmax_j e_ij      alpha~ = alpha * mult      out_i = sum_j alpha~_ij x_l[j]
// the gradients are
//     dalpha_ij = mult_ij <dout_i, x_l[j]>      de_ij = alpha_ij (dalpha_ij - sum_j' alpha_ij' dalpha_ij')
//     d x_r[i] += de_ij att (.) lrelu'(s)      d att += de_ij lrelu(s)      d x_l[j] += alpha~_ij dout_i + de_ij att (.) lrelu'(s)
// with s = x_l[j] + x_r[i].  Which lanes walk which edges, and where a column index comes from, stays with the kernels.
#pragma once
#include "spatial_common.h"

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

namespace tecm_spatial {

constexpr int TB = 256;                 // threads of a block of the rows / target / source kernels (spatial_dx, spatial_attn)
constexpr int HP = 12;                  // floats per head in a 24-float row: 11 channels | u, norm or pad
constexpr int64_t WS_CHUNK_BYTES = (int64_t)64 << 20;   // workspace of one chunk of graphs (spatial_dx, spatial_attn)

__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ f32x16 splat16(float v) {
  f32x16 a;
#pragma unroll
  for (int e = 0; e < 16; ++e) a[e] = v;
  return a;
}

// one head of a 24-float row (16-byte aligned): 11 channels and the float behind them (u, norm or pad)
__device__ __forceinline__ void ld12(const float* p, float (&v)[CH + 1]) {
  const float4* q = reinterpret_cast<const float4*>(p);
  const float4 a = q[0], b = q[1], c = q[2];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
}
__device__ __forceinline__ void st12(float* p, const float (&v)[CH], float last) {
  float4* q = reinterpret_cast<float4*>(p);
  q[0] = make_float4(v[0], v[1], v[2], v[3]);
  q[1] = make_float4(v[4], v[5], v[6], v[7]);
  q[2] = make_float4(v[8], v[9], v[10], last);
}

// ---- dropout of the attention coefficients: the mask of (row of the (L*B*N) flattening, head, slot in the target's list)
struct AlphaDrop {
  uint32_t th;                          // 0: no dropout
  float inv;
};
__device__ __forceinline__ AlphaDrop alpha_drop_of(const TecmSpatial& d) {
  AlphaDrop a;
  a.th = d.alpha_drop.p > 0.f ? tecm_drop_thresh(d.alpha_drop.p) : 0u;
  a.inv = d.alpha_drop.p > 0.f ? 1.0f / (1.0f - d.alpha_drop.p) : 1.0f;
  return a;
}
__device__ __forceinline__ uint64_t alpha_drop_seed(const TecmSpatial& d) {
  return tecm_seed_now(d.alpha_drop.seed, d.alpha_drop.seed_dev);
}
__device__ __forceinline__ uint64_t alpha_drop_base(const TecmSpatial& d, int64_t row, int head) {
  return (uint64_t)((row * H + head) * d.alpha_drop.ld);
}
__device__ __forceinline__ float alpha_drop_mult(const AlphaDrop& a, uint64_t seed, uint64_t idx) {
  return tecm_drop_mult(seed, idx, a.th, a.inv);
}

// ---- the logit.  Packed |.| form (forward kernels), scaled by log2(e): att4 = 0.4 log2e att, base = 0.6 log2e u_r,
//      a[CH] = u_l; s = x_l[j] + x_r[i] two channels at a time (v_pk_add_f32)
__device__ __forceinline__ float logit_abs(const float (&a)[CH + 1], const float (&xr)[CH + 1], const float (&att4)[CH],
                                           float base) {
  float e = fmaf(0.6f * LOG2E, a[CH], base);
#pragma unroll
  for (int c = 0; c + 1 < CH; c += 2) {
    const f32x2 sv = f32x2{a[c], a[c + 1]} + f32x2{xr[c], xr[c + 1]};
    e = fmaf(att4[c], fabsf(sv.x), e);
    e = fmaf(att4[c + 1], fabsf(sv.y), e);
  }
  return fmaf(att4[CH - 1], fabsf(a[CH - 1] + xr[CH - 1]), e);
}
// <g, a> with even and odd channels in separate chains
__device__ __forceinline__ float dot11_eo(const float (&g)[CH + 1], const float (&a)[CH + 1]) {
  float da = 0.f, db = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (c & 1) db = fmaf(g[c], a[c], db);
    else da = fmaf(g[c], a[c], da);
  }
  return da + db;
}
// The same logit (att unscaled) with dalpha = <g, x_l[j]> beside it (backward kernels), even / odd channels in separate chains
__device__ __forceinline__ float logit_dalpha(const float (&a)[CH + 1], const float (&xr)[CH + 1], const float (&g)[CH + 1],
                                              const float (&att)[CH], float base, float& dalpha) {
  float t0 = 0.f, u0 = 0.f, da = 0.f, db = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (c & 1) {
      u0 = fmaf(att[c], fabsf(a[c] + xr[c]), u0);
      db = fmaf(g[c], a[c], db);
    } else {
      t0 = fmaf(att[c], fabsf(a[c] + xr[c]), t0);
      da = fmaf(g[c], a[c], da);
    }
  }
  dalpha = da + db;
  return fmaf(0.4f * LOG2E, t0 + u0, fmaf(0.6f * LOG2E, a[CH], base));
}
// Plain form, natural units (input gradient, attention export): rows without u
__device__ __forceinline__ float logit_lrelu(const float (&xl)[CH + 1], const float (&xr)[CH + 1], const float (&att)[CH]) {
  float e = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) e = fmaf(att[c], lrelu(xl[c] + xr[c]), e);
  return e;
}
template <int NA, int NB>
__device__ __forceinline__ float dot11(const float (&a)[NA], const float (&b)[NB]) {
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) v = fmaf(a[c], b[c], v);
  return v;
}

// ---- one online-softmax step.  Scalar form: (mx, z, num) <- (e, da); scale = 1 for a logit in base-2 units, LOG2E for one
//      in natural units
__device__ __forceinline__ void softmax_step(float e, float da, float scale, float& mx, float& z, float& num) {
  const float mn = fmaxf(mx, e);
  const float corr = __builtin_amdgcn_exp2f((mx - mn) * scale), pw = __builtin_amdgcn_exp2f((e - mn) * scale);
  z = fmaf(z, corr, pw);
  num = fmaf(num, corr, pw * da);
  mx = mn;
}
// EU slots per step with ONE rescale of the accumulators: a[u] = x_l row of slot u, ev[u] its logit (-inf: no such slot;
// slot 0 is always valid, so the new maximum is finite), didx = mask index of slot 0
template <int EU>
__device__ __forceinline__ void softmax_step(const float (&a)[EU][CH + 1], const float (&ev)[EU], const AlphaDrop& dr,
                                             uint64_t dseed, uint64_t didx, float& m, float& z, float (&acc)[CH + 1]) {
  float mn = m;
#pragma unroll
  for (int u = 0; u < EU; ++u) mn = fmaxf(mn, ev[u]);
  const float corr = __builtin_amdgcn_exp2f(m - mn);         // exp2(-inf) = 0 on the first step
  float pm[EU], zs = 0.f;
#pragma unroll
  for (int u = 0; u < EU; ++u) {
    const float p = __builtin_amdgcn_exp2f(ev[u] - mn);
    zs += p;
    pm[u] = p;
    if (dr.th) pm[u] = p * alpha_drop_mult(dr, dseed, didx + u);
  }
  z = z * corr + zs;
  m = mn;
#pragma unroll
  for (int c = 0; c < CH + 1; c += 2) {                      // channel pairs (the 12th lane of the pair is the unused u)
    f32x2 t = f32x2{acc[c], acc[c + 1]} * corr;
#pragma unroll
    for (int u = 0; u < EU; ++u) t = f32x2{a[u][c], a[u][c + 1]} * pm[u] + t;
    acc[c] = t.x;
    acc[c + 1] = t.y;
  }
}

// ---- what an edge's de adds: to d x_r[i] (and d att), to d x_l[j] (with the message term alpha~ dout_i)
template <int NA, int NB>
__device__ __forceinline__ void de_to_dxr(float de, const float (&xl)[NA], const float (&xr)[NB], const float (&att)[CH],
                                          float (&dxr)[CH]) {
#pragma unroll
  for (int c = 0; c < CH; ++c) dxr[c] = fmaf(de, xl[c] + xr[c] > 0.f ? att[c] : NEG_SLOPE * att[c], dxr[c]);
}
__device__ __forceinline__ void de_to_dxr_datt(float de, const float (&xl)[CH + 1], const float (&xr)[CH + 1],
                                               const float (&att)[CH], float (&dxr)[CH], float (&datt)[CH]) {
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const float sv = xl[c] + xr[c];
    const bool pos = sv > 0.f;
    dxr[c] = fmaf(de, pos ? att[c] : NEG_SLOPE * att[c], dxr[c]);
    datt[c] = fmaf(de, pos ? sv : NEG_SLOPE * sv, datt[c]);
  }
}
template <int NG, int NA, int NB>
__device__ __forceinline__ void de_to_dxl(float am, float de, const float (&g)[NG], const float (&xl)[NA], const float (&xr)[NB],
                                          const float (&att)[CH], float (&dxl)[CH]) {
#pragma unroll
  for (int c = 0; c < CH; ++c) dxl[c] = fmaf(am, g[c], fmaf(de, xl[c] + xr[c] > 0.f ? att[c] : NEG_SLOPE * att[c], dxl[c]));
}

}  // namespace tecm_spatial
