// The element math of GroupNorm(1) + GELU (Multi_Scale_Conv_Block, modules.py:28-29), once, for every kernel of
// groupnorm.hip: scalar functions the quad (float4) and oct (8-channel) kernels call per component, the 16-byte loads and
// stores of those units and the reduction over the waves of a sequence.  With y_hat = (y - mean) * rstd and
// act = gelu(y_hat * gamma + beta) the gradients are
//     g = dact * gelu'(y_hat * gamma + beta)      d gamma += g * y_hat      d beta += g      d = g * gamma
//     dy = rstd * (d - mean(d) - y_hat * mean(d * y_hat))
// with the means over the sequence's branch.  Which lane holds which element, and every accumulator, stays with the kernels.
// The expressions are written in ONE order (the compiler contracts the same multiply-adds everywhere): results are
// bit-identical between kernels that see the same values in the same summation order.
#pragma once
#include "common.h"

namespace tecm_gn {

// GELU flavour: libm's erff in the generic rows kernels, the one-exponential form (common.h) everywhere else
enum class Gelu { Erf, Fast };

template <Gelu F>
__device__ __forceinline__ float gelu(float v) {
  if constexpr (F == Gelu::Erf) return gelu_erf(v);
  else return gelu_erf_fast(v);
}
template <Gelu F>
__device__ __forceinline__ float dgelu(float v) {
#ifdef GN_ABLATE_DGELU                                    // diagnostics (tools/build_variant.py): no transcendental in any backward
  return 0.5f + 0.1f * v;
#else
  if constexpr (F == Gelu::Erf) return dgelu_erf(v);
  else return dgelu_erf_fast(v);
#endif
}

__device__ __forceinline__ float y_hat(float y, float mean, float rstd) { return (y - mean) * rstd; }

// forward element
template <Gelu F>
__device__ __forceinline__ float fwd_elem(float y, float mean, float rstd, float gamma, float beta) {
  return gelu<F>((y - mean) * rstd * gamma + beta);
}

// backward element: h = y_hat, g = the gradient at the affine output (what d gamma / d beta sum), d() = the gradient at
// y_hat -- a member function, so that the product is formed where the caller first asks for it: behind its d gamma /
// d beta updates, the statement order the instruction scheduler has always been given
struct BwdElem {
  float h, g, gamma;
  __device__ __forceinline__ float d() const { return g * gamma; }
};
template <Gelu F>
__device__ __forceinline__ BwdElem bwd_elem(float y, float dact, float mean, float rstd, float gamma, float beta) {
  BwdElem r;
  r.h = y_hat(y, mean, rstd);
  r.g = dact * dgelu<F>(r.h * gamma + beta);
  r.gamma = gamma;
  return r;
}

// output element: m1 = mean(d), m2 = mean(d * y_hat) over the sequence's branch
__device__ __forceinline__ float dy_elem(float rstd, float d, float m1, float m2, float h) { return rstd * (d - m1 - h * m2); }

// ---- a quad of the (B, L, N, 3*Cout) conv tensors: fp32, or -- the kernels' OUTPUTS in bf16 mode (BASELINE configs[2]) --
// bf16: act and dy only feed bf16 contractions, which would round them in their loaders.  Offsets are in elements.
template <bool h16>
__device__ __forceinline__ float4 gn_ld4(const void* p, int64_t off) {
  if constexpr (h16) {
    const tecm_bf16x4 v = *reinterpret_cast<const tecm_bf16x4*>(reinterpret_cast<const __bf16*>(p) + off);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  }
  return *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + off);
}
template <bool h16>
__device__ __forceinline__ void gn_st4(void* p, int64_t off, const float4& v) {
  if constexpr (h16) tecm_store_bf16x4(reinterpret_cast<__bf16*>(p) + off, v.x, v.y, v.z, v.w);
  else *reinterpret_cast<float4*>(reinterpret_cast<float*>(p) + off) = v;
}

// ---- an oct: 8 consecutive bf16 channels = one 16-byte load / store (gamma / beta: two fp32 quads)
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8n __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x8 gn_ld8(const void* p, int64_t off) {
  const bf16x8n v = *reinterpret_cast<const bf16x8n*>(reinterpret_cast<const __bf16*>(p) + off);
  f32x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (float)v[e];
  return r;
}
__device__ __forceinline__ void gn_st8(void* p, int64_t off, const f32x8& v) {
  bf16x8n h;
#pragma unroll
  for (int e = 0; e < 8; ++e) h[e] = (__bf16)v[e];
  *reinterpret_cast<bf16x8n*>(reinterpret_cast<__bf16*>(p) + off) = h;
}
__device__ __forceinline__ f32x8 gn_ld8f(const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  f32x8 r = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return r;
}

__device__ __forceinline__ float sel3(int k, float a, float b, float c) { return k == 0 ? a : (k == 1 ? b : c); }
__device__ __forceinline__ float sum4(const float4& v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float sum8(const f32x8& v) { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); }

// sums over the WPS waves of a sequence: xch[wave][3], waves of one sequence are consecutive.  The order of the sum fixes
// the last bits of every statistic, so each wave count keeps the one it has always had: six waves (the oct kernels,
// whose block is one sequence) add in pairs, ((0 + 1) + (2 + 3)) + (4 + 5); every other count adds left to right.
template <int WPS>
__device__ __forceinline__ void seq_reduce3(float (&v)[3], float (*xch)[3], int wave, int lane) {
#pragma unroll
  for (int b = 0; b < 3; ++b) v[b] = wave_sum(v[b]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int b = 0; b < 3; ++b) xch[wave][b] = v[b];
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    if constexpr (WPS == 6) {                             // the block is the sequence
      v[b] = ((xch[0][b] + xch[1][b]) + (xch[2][b] + xch[3][b])) + (xch[4][b] + xch[5][b]);
    } else {
      const int w0 = wave / WPS * WPS;
      float t = xch[w0][b];
#pragma unroll
      for (int w = 1; w < WPS; ++w) t += xch[w0 + w][b];
      v[b] = t;
    }
  }
}

}  // namespace tecm_gn
