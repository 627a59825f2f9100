// LayerNorm forward / backward of the TEC-MoLLM path (gfx950, wave = 64): GPT2Block.ln_1 / ln_2 / ln_f
// (modeling_gpt2.py:262-310, :620).  Bandwidth-bound: one wave owns one row, statistics are wave reductions, the gamma /
// beta gradients are kept in registers across the rows a wave visits and leave the kernel as one partial row per block
// (summed by tecm_colsum, colsum.hip) -- no atomics, deterministic.
#include "norm_common.h"

namespace {

constexpr int LN_MAXCH = 4;  // float4 chunks per lane: D <= 1024

// ------------------------------------------------------------------------------ LayerNorm
template <int NCH>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const float* __restrict__ x, int64_t ldx,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ y,
                                                            int64_t ldy, void* __restrict__ y16, int64_t ldy16,
                                                            void* __restrict__ y16d, int64_t ldy16d, DropCtxN dd,
                                                            float* __restrict__ stats, int64_t M, int D, float eps,
                                                            int permT, int permN, int yd_f32) {
  seed_now(dd);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= M) return;
  // y16d may be written SEQUENCE-major: time-major row (b, t, n) -> row (b, n, t), i.e. PredictionHead's view(batch, -1)
  // (modules.py:307) of the (B*N, T, D) hidden state as a plain [B*N][T*D] matrix (the mask index stays the time-major one)
  int64_t drow = row;
  if (permT > 0) {
    const int64_t tn = (int64_t)permT * permN;
    const int64_t b = row / tn, rem = row - b * tn;
    const int64_t t = rem / permN, n = rem - t * permN;
    drow = (b * permN + n) * permT + t;
  }
  const float* xr = x + row * ldx;
  float4 v[NCH];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = 4 * (lane + 64 * i);
    v[i] = c < D ? *reinterpret_cast<const float4*>(xr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = 4 * (lane + 64 * i);
    if (c < D) {
      const float a = v[i].x - mean, b = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
      q += (a * a + b * b) + (cc * cc + d * d);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = 4 * (lane + 64 * i);
    if (c < D) {
      const float4 g = *reinterpret_cast<const float4*>(gamma + c);
      const float4 b = *reinterpret_cast<const float4*>(beta + c);
      float4 o;
      o.x = (v[i].x - mean) * rstd * g.x + b.x;
      o.y = (v[i].y - mean) * rstd * g.y + b.y;
      o.z = (v[i].z - mean) * rstd * g.z + b.z;
      o.w = (v[i].w - mean) * rstd * g.w + b.w;
      if (y) *reinterpret_cast<float4*>(y + row * ldy + c) = o;
      // bf16 copy for a bf16 matrix-core GEMM that only ever reads the rounded value (rounded once here)
      if (y16) tecm_store_bf16x4(static_cast<__bf16*>(y16) + row * ldy16 + c, o.x, o.y, o.z, o.w);
      // ... and bf16(dropout(o)): the LoRA branch's input (peft lora_dropout in front of lora_A, modules.py:181), the
      // cast autocast applies to the DROPPED fp32 value; read by the LoRA-A GEMM and by its weight gradient
      // (yd_f32: the same output left in fp32 -- fp32 mode's head operand, dropout(ln_f(h)) sequence-major: what
      //  tecm_dropout_apply would make of y, without y or that pass)
      if (y16d) {
        const uint64_t di = (uint64_t)(row * dd.ld + c);
        const float m0 = o.x * tecm_drop_mult(dd.seed, di, dd.thresh, dd.inv);
        const float m1 = o.y * tecm_drop_mult(dd.seed, di + 1, dd.thresh, dd.inv);
        const float m2 = o.z * tecm_drop_mult(dd.seed, di + 2, dd.thresh, dd.inv);
        const float m3 = o.w * tecm_drop_mult(dd.seed, di + 3, dd.thresh, dd.inv);
        if (yd_f32) *reinterpret_cast<float4*>(static_cast<float*>(y16d) + drow * ldy16d + c) = make_float4(m0, m1, m2, m3);
        else tecm_store_bf16x4(static_cast<__bf16*>(y16d) + drow * ldy16d + c, m0, m1, m2, m3);
      }
    }
  }
  if (lane == 0) {
    stats[2 * row] = mean;
    stats[2 * row + 1] = rstd;
  }
}

// Optional SECOND gradient stream of the same tensor: dy2 (M, D), fp32 or bf16, times an optional dropout mask -- the gradient
// the LoRA branch of peft's c_attn returns for ITS input (lora_A's d-input GEMM, modules.py:177-186), which reaches the
// LayerNorm output through lora_dropout's backward (modules.py:181):     dy[row][c] += keep(row, c) / (1 - p) * dy2[row][c].
// (Round 4 first folded the rank-32 product itself into this kernel -- lora_A in LDS, one 1024-thread block per CU -- and
// measured 370 us per launch against 148 + 129 for this kernel plus the K = 32 GEMM: the LDS image costs the occupancy a
// bandwidth kernel lives on.  The product stays a GEMM, its read-modify-write of the M x D gradient is what went away.)
struct LnAdd {
  const void* dy2;
  int64_t ld;
  int32_t bf16, _pad;
  DropCtxN drop;
};

// DY16: dy is a bf16 matrix (bf16 mode: the gradient a bf16 Linear hands back for its input, train.py:68)
// DYMAP (dy bf16 or fp32): that matrix is SEQUENCE-major -- row (b, n, t) for the time-major row (b, t, n) this kernel walks --
// and still in front of a dropout: dy[row][c] = keep(row, c) / (1 - p) * dy[(b, n, t)][c].  The gradient the head's first
// Linear returns for F.dropout(hidden) (tec_mollm.py:115, modules.py:307), consumed by ln_f's backward without a pass of
// its own for the mask or the layout.
struct LnDyMap {
  int T, N;
  DropCtxN drop;
};
template <int NCH, bool ADD, bool DY16 = false, bool DYMAP = false>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ dy, int64_t lddy,
                                                            const float* __restrict__ x, int64_t ldx,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ stats,
                                                            const float* __restrict__ dres, float* __restrict__ dx,
                                                            float* __restrict__ dxm, int dxm_bf16, DropCtxN odc,
                                                            float* __restrict__ partials, int64_t M, int D, LnAdd ad,
                                                            LnDyMap dm = LnDyMap{}) {
  seed_now(odc);
  seed_now(ad.drop);
  seed_now(dm.drop);
  __shared__ float red[4][2 * 4 * 64 * NCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 dg[NCH], db[NCH], gm[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    dg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    db[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int c = 4 * (lane + 64 * i);
    gm[i] = c < D ? *reinterpret_cast<const float4*>(gamma + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float invD = 1.0f / (float)D;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < M; row += (int64_t)gridDim.x * 4) {
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    float4 xh[NCH], g[NCH];
    float s1 = 0.f, s2 = 0.f;
    int64_t yrow = row;
    if constexpr (DYMAP) {
      const int64_t tn = (int64_t)dm.T * dm.N;
      const int64_t b = row / tn, rem = row - b * tn;
      const int64_t t = rem / dm.N, n = rem - t * dm.N;
      yrow = (b * dm.N + n) * dm.T + t;
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = 4 * (lane + 64 * i);
      if (c < D) {
        const float4 xv = *reinterpret_cast<const float4*>(x + row * ldx + c);
        float4 d;
        if constexpr (DY16) {
          const tecm_bf16x4 h = *reinterpret_cast<const tecm_bf16x4*>(reinterpret_cast<const __bf16*>(dy) + yrow * lddy + c);
          d = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
        } else {
          d = *reinterpret_cast<const float4*>(dy + yrow * lddy + c);
        }
        if constexpr (DYMAP) {
          if (dm.drop.thresh) {
            const uint64_t di = (uint64_t)(row * dm.drop.ld + c);
            d.x *= tecm_drop_mult(dm.drop.seed, di, dm.drop.thresh, dm.drop.inv);
            d.y *= tecm_drop_mult(dm.drop.seed, di + 1, dm.drop.thresh, dm.drop.inv);
            d.z *= tecm_drop_mult(dm.drop.seed, di + 2, dm.drop.thresh, dm.drop.inv);
            d.w *= tecm_drop_mult(dm.drop.seed, di + 3, dm.drop.thresh, dm.drop.inv);
          }
        }
        if constexpr (ADD) {
          float4 e;
          if (ad.bf16) {
            const tecm_bf16x4 h = *reinterpret_cast<const tecm_bf16x4*>(reinterpret_cast<const __bf16*>(ad.dy2) + row * ad.ld + c);
            e = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
          } else {
            e = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(ad.dy2) + row * ad.ld + c);
          }
          if (ad.drop.thresh) {
            const uint64_t di = (uint64_t)(row * ad.drop.ld + c);
            e.x *= tecm_drop_mult(ad.drop.seed, di, ad.drop.thresh, ad.drop.inv);
            e.y *= tecm_drop_mult(ad.drop.seed, di + 1, ad.drop.thresh, ad.drop.inv);
            e.z *= tecm_drop_mult(ad.drop.seed, di + 2, ad.drop.thresh, ad.drop.inv);
            e.w *= tecm_drop_mult(ad.drop.seed, di + 3, ad.drop.thresh, ad.drop.inv);
          }
          d.x += e.x; d.y += e.y; d.z += e.z; d.w += e.w;
        }
        xh[i] = make_float4((xv.x - mean) * rstd, (xv.y - mean) * rstd, (xv.z - mean) * rstd, (xv.w - mean) * rstd);
        g[i] = make_float4(d.x * gm[i].x, d.y * gm[i].y, d.z * gm[i].z, d.w * gm[i].w);
        dg[i].x += d.x * xh[i].x; dg[i].y += d.y * xh[i].y; dg[i].z += d.z * xh[i].z; dg[i].w += d.w * xh[i].w;
        db[i].x += d.x; db[i].y += d.y; db[i].z += d.z; db[i].w += d.w;
        s1 += (g[i].x + g[i].y) + (g[i].z + g[i].w);
        s2 += (g[i].x * xh[i].x + g[i].y * xh[i].y) + (g[i].z * xh[i].z + g[i].w * xh[i].w);
      } else {
        xh[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        g[i] = xh[i];
      }
    }
    s1 = wave_sum(s1) * invD;
    s2 = wave_sum(s2) * invD;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = 4 * (lane + 64 * i);
      if (c < D) {
        float o[4] = {rstd * (g[i].x - s1 - xh[i].x * s2), rstd * (g[i].y - s1 - xh[i].y * s2),
                      rstd * (g[i].z - s1 - xh[i].z * s2), rstd * (g[i].w - s1 - xh[i].w * s2)};
        if (dres) {
          const float4 r = *reinterpret_cast<const float4*>(dres + row * (int64_t)D + c);
          o[0] += r.x; o[1] += r.y; o[2] += r.z; o[3] += r.w;
        }
        if (dx) *reinterpret_cast<float4*>(dx + row * (int64_t)D + c) = make_float4(o[0], o[1], o[2], o[3]);
        if (dxm) {          // second output: dropout(dx) for the GEMM that consumes the masked gradient
          if (odc.thresh) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              o[e] *= tecm_drop_mult(odc.seed, (uint64_t)(row * odc.ld + c + e), odc.thresh, odc.inv);
          }
          if (dxm_bf16)
            tecm_store_bf16x4(reinterpret_cast<__bf16*>(dxm) + row * (int64_t)D + c, o[0], o[1], o[2], o[3]);
          else
            *reinterpret_cast<float4*>(dxm + row * (int64_t)D + c) = make_float4(o[0], o[1], o[2], o[3]);
        }
      }
    }
  }
  // block reduction of the per-lane parameter gradients -> one partial row per block
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = 4 * (lane + 64 * i);
    float* r0 = &red[wave][c];
    float* r1 = &red[wave][4 * 64 * NCH + c];
    r0[0] = dg[i].x; r0[1] = dg[i].y; r0[2] = dg[i].z; r0[3] = dg[i].w;
    r1[0] = db[i].x; r1[1] = db[i].y; r1[2] = db[i].z; r1[3] = db[i].w;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * D; c += 256) {
    const int src = c < D ? c : (4 * 64 * NCH + (c - D));
    partials[(int64_t)blockIdx.x * 2 * D + c] = (red[0][src] + red[1][src]) + (red[2][src] + red[3][src]);
  }
}

int ln_blocks(int64_t M) {
  const int64_t want = (M + 3) / 4;
  return (int)(want < 1024 ? want : 1024);
}

}  // namespace

extern "C" int tecm_layernorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, float* y,
                                  int64_t ldy, void* y16, int64_t ldy16, void* y16d, int64_t ldy16d, const TecmDrop* drop,
                                  int32_t y16d_seq_T, int32_t y16d_seq_N, int32_t y16d_f32, float* stats, int64_t M, int32_t D,
                                  float eps, void* stream) {
  TECM_REQUIRE(x && gamma && beta && (y || y16 || y16d) && stats, TECM_E_ARG, "tecm_layernorm_fwd: null pointer");
  TECM_REQUIRE(y16d_seq_T == 0 || (y16d && y16d_seq_T > 0 && y16d_seq_N > 0 && M % ((int64_t)y16d_seq_T * y16d_seq_N) == 0),
               TECM_E_ARG, "tecm_layernorm_fwd: the sequence-major form needs y16d and M = B * T * N");
  TECM_REQUIRE(!y16d || (tecm_aligned(y16d, y16d_f32 ? 16 : 8) && ldy16d % 4 == 0 && ldy16d >= D), TECM_E_ALIGN,
               "tecm_layernorm_fwd: the dropped output must be 8-byte (bf16) / 16-byte (fp32) aligned with a leading dimension "
               "multiple of 4");
  TECM_REQUIRE(!y16d_f32 || y16d, TECM_E_ARG, "tecm_layernorm_fwd: y16d_f32 goes with y16d");
  TECM_REQUIRE(!y16d || (drop && drop->p >= 0.f && drop->p < 1.f), TECM_E_ARG, "tecm_layernorm_fwd: y16d needs its dropout spec");
  const DropCtxN dd = make_dropn(y16d ? drop : nullptr);
  TECM_REQUIRE(!y16 || (tecm_aligned(y16, 8) && ldy16 % 4 == 0 && ldy16 >= D), TECM_E_ALIGN,
               "tecm_layernorm_fwd: the bf16 output must be 8-byte aligned with a leading dimension multiple of 4");
  TECM_REQUIRE(M > 0 && D > 0 && D % 4 == 0 && D <= 256 * LN_MAXCH, TECM_E_ARG,
               "tecm_layernorm_fwd: need D %% 4 == 0 and D <= %d (got %d)", 256 * LN_MAXCH, D);
  TECM_REQUIRE(ldx % 4 == 0 && (!y || (ldy % 4 == 0 && tecm_aligned(y, 16))) && tecm_aligned(x, 16) &&
                   tecm_aligned(gamma, 16) && tecm_aligned(beta, 16),
               TECM_E_ALIGN, "tecm_layernorm_fwd: 16-byte alignment required");
  const dim3 grid((unsigned)((M + 3) / 4));
  const int nch = (D + 255) / 256;
  hipStream_t st = (hipStream_t)stream;
#define LN_FWD(NCH) \
  hipLaunchKernelGGL((layernorm_fwd_kernel<NCH>), grid, dim3(256), 0, st, x, ldx, gamma, beta, y, ldy, y16, ldy16, y16d, ldy16d, \
                     dd, stats, M, D, eps, (int)y16d_seq_T, (int)y16d_seq_N, (int)(y16d_f32 != 0))
  switch (nch) {
    case 1: LN_FWD(1); break;
    case 2: LN_FWD(2); break;
    case 3: LN_FWD(3); break;
    default: LN_FWD(4); break;
  }
#undef LN_FWD
  TECM_CHECK_LAUNCH("tecm_layernorm_fwd");
  return TECM_OK;
}

extern "C" int tecm_layernorm_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma,
                                  const float* stats, const float* dres, float* dx, void* dx_masked,
                                  int32_t masked_bf16, const TecmDrop* mask_drop, float* dgb_partials,
                                  int32_t* num_blocks, int64_t M, int32_t D, const TecmLnAdd* add, int32_t dy_bf16,
                                  const TecmLnDyMap* dymap, int32_t skip_dx, void* stream) {
  TECM_REQUIRE(M > 0 && D > 0 && D % 4 == 0 && D <= 256 * LN_MAXCH, TECM_E_ARG, "tecm_layernorm_bwd: bad M/D");
  const int nb = ln_blocks(M);
  if (num_blocks) *num_blocks = nb;
  if (dx == nullptr) return TECM_OK;   // query mode
  TECM_REQUIRE(dy && x && gamma && stats && dgb_partials, TECM_E_ARG, "tecm_layernorm_bwd: null pointer");
  TECM_REQUIRE(lddy % 4 == 0 && ldx % 4 == 0 && tecm_aligned(dy, dy_bf16 ? 8 : 16) && tecm_aligned(x, 16) &&
                   tecm_aligned(dx, 16) && (!dres || tecm_aligned(dres, 16)) &&
                   (!dx_masked || tecm_aligned(dx_masked, 16)),
               TECM_E_ALIGN, "tecm_layernorm_bwd: 16-byte alignment required");
  const DropCtxN odc = make_dropn(mask_drop);
  const int nch = (D + 255) / 256;
  hipStream_t st = (hipStream_t)stream;
  LnAdd ad{};
  const bool has_add = add != nullptr && add->dy2 != nullptr;
  if (has_add) {
    TECM_REQUIRE(add->ld % 4 == 0 && add->ld >= D && tecm_aligned(add->dy2, add->bf16 ? 8 : 16), TECM_E_ALIGN,
                 "tecm_layernorm_bwd: dy2 must be 16-byte (fp32) / 8-byte (bf16) friendly");
    ad.dy2 = add->dy2; ad.ld = add->ld; ad.bf16 = add->bf16; ad.drop = make_dropn(&add->drop);
  }
 LnDyMap dm{};
  const bool has_map = dymap != nullptr && dymap->T > 0;
  if (has_map) {
    TECM_REQUIRE(!has_add && dymap->N > 0 && M % ((int64_t)dymap->T * dymap->N) == 0, TECM_E_ARG,
                 "tecm_layernorm_bwd: the sequence-major dy is a matrix of M = B * T * N rows, without a second stream");
    dm.T = dymap->T; dm.N = dymap->N; dm.drop = make_dropn(&dymap->drop);
  }
  // skip_dx: the unmasked dx has no reader (dx_masked is the only output): its store is left out, dx is not touched
  TECM_REQUIRE(!skip_dx || dx_masked, TECM_E_ARG, "tecm_layernorm_bwd: skip_dx needs dx_masked");
  if (skip_dx) dx = nullptr;
#define LN_BWD(NCH)                                                                                                       \
  do {                                                                                                                    \
    if (has_map && dy_bf16)                                                                                               \
      hipLaunchKernelGGL((layernorm_bwd_kernel<NCH, false, true, true>), dim3(nb), dim3(256), 0, st, dy, lddy, x, ldx, gamma, \
                         stats, dres, dx, static_cast<float*>(dx_masked), (int)masked_bf16, odc, dgb_partials, M, D, ad, dm); \
    else if (has_map)                                                                                                     \
      hipLaunchKernelGGL((layernorm_bwd_kernel<NCH, false, false, true>), dim3(nb), dim3(256), 0, st, dy, lddy, x, ldx, gamma, \
                         stats, dres, dx, static_cast<float*>(dx_masked), (int)masked_bf16, odc, dgb_partials, M, D, ad, dm); \
    else if (has_add && dy_bf16)                                                                                               \
      hipLaunchKernelGGL((layernorm_bwd_kernel<NCH, true, true>), dim3(nb), dim3(256), 0, st, dy, lddy, x, ldx, gamma, stats, \
                         dres, dx, static_cast<float*>(dx_masked), (int)masked_bf16, odc, dgb_partials, M, D, ad);        \
    else if (has_add)                                                                                                     \
      hipLaunchKernelGGL((layernorm_bwd_kernel<NCH, true, false>), dim3(nb), dim3(256), 0, st, dy, lddy, x, ldx, gamma, stats, \
                         dres, dx, static_cast<float*>(dx_masked), (int)masked_bf16, odc, dgb_partials, M, D, ad);        \
    else if (dy_bf16)                                                                                                     \
      hipLaunchKernelGGL((layernorm_bwd_kernel<NCH, false, true>), dim3(nb), dim3(256), 0, st, dy, lddy, x, ldx, gamma, stats, \
                         dres, dx, static_cast<float*>(dx_masked), (int)masked_bf16, odc, dgb_partials, M, D, ad);        \
    else                                                                                                                  \
      hipLaunchKernelGGL((layernorm_bwd_kernel<NCH, false, false>), dim3(nb), dim3(256), 0, st, dy, lddy, x, ldx, gamma, stats, \
                         dres, dx, static_cast<float*>(dx_masked), (int)masked_bf16, odc, dgb_partials, M, D, ad);        \
  } while (0)
  switch (nch) {
    case 1: LN_BWD(1); break;
    case 2: LN_BWD(2); break;
    case 3: LN_BWD(3); break;
    default: LN_BWD(4); break;
  }
#undef LN_BWD
  TECM_CHECK_LAUNCH("tecm_layernorm_bwd");
  return TECM_OK;
}
