// GroupNorm(1) + GELU of the Multi_Scale_Conv_Block branches (modules.py:28-29), the three branches at once (gfx950,
// wave = 64).  Bandwidth-bound: one wave (generic rows kernels) or a few waves (register-resident kernels) own one
// sequence; statistics are wave reductions, per-channel parameter gradients are kept in registers across the sequences a
// block visits and leave the kernel as one partial row per block (summed by tecm_colsum) -- no atomics, deterministic.
// The element math of every kernel is gn_math.h; which kernel serves a call is decided by gn_fwd_plan / gn_bwd_plan.
#include <type_traits>

#include "gn_math.h"

namespace {

using namespace tecm_gn;

// ------------------------------------------------------------------------------ GroupNorm(1) + GELU
// CPB = Cout / 64 (channel chunks of 64 per branch); lane owns channels lane + 64*i.
template <int CPB>
__global__ __launch_bounds__(256) void gn_gelu_fwd_kernel(const float* __restrict__ y, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ act,
                                                          float* __restrict__ stats, int B, int L, int N, float eps) {
  constexpr int CT = 3 * CPB * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t sidx = (int64_t)blockIdx.x * 4 + wave;
  if (sidx >= (int64_t)B * N) return;
  const int b = (int)(sidx / N), n = (int)(sidx - (int64_t)b * N);
  const float inv_cnt = 1.0f / (float)(L * CPB * 64);
  const int64_t tstride = (int64_t)N * CT;
  const float* base = y + ((int64_t)b * L * N + n) * CT + lane;
  float mean[3], rstd[3];
  {
    float s[3] = {0.f, 0.f, 0.f};
    for (int t = 0; t < L; ++t) {
      const float* p = base + t * tstride;
#pragma unroll
      for (int br = 0; br < 3; ++br)
#pragma unroll
        for (int k = 0; k < CPB; ++k) s[br] += p[64 * (br * CPB + k)];
    }
#pragma unroll
    for (int br = 0; br < 3; ++br) mean[br] = wave_sum(s[br]) * inv_cnt;
  }
  {
    float s[3] = {0.f, 0.f, 0.f};
    for (int t = 0; t < L; ++t) {
      const float* p = base + t * tstride;
#pragma unroll
      for (int br = 0; br < 3; ++br)
#pragma unroll
        for (int k = 0; k < CPB; ++k) {
          const float d = p[64 * (br * CPB + k)] - mean[br];
          s[br] += d * d;
        }
    }
#pragma unroll
    for (int br = 0; br < 3; ++br) rstd[br] = 1.0f / sqrtf(wave_sum(s[br]) * inv_cnt + eps);
  }
  float gm[3 * CPB], bt[3 * CPB];
#pragma unroll
  for (int i = 0; i < 3 * CPB; ++i) {
    gm[i] = gamma[lane + 64 * i];
    bt[i] = beta[lane + 64 * i];
  }
  float* obase = act + ((int64_t)b * L * N + n) * CT + lane;
  for (int t = 0; t < L; ++t) {
    const float* p = base + t * tstride;
    float* o = obase + t * tstride;
#pragma unroll
    for (int br = 0; br < 3; ++br)
#pragma unroll
      for (int k = 0; k < CPB; ++k) {
        const int i = br * CPB + k;
        o[64 * i] = fwd_elem<Gelu::Erf>(p[64 * i], mean[br], rstd[br], gm[i], bt[i]);
      }
  }
  if (lane < 3) {
    stats[(sidx * 3 + lane) * 2] = mean[lane];
    stats[(sidx * 3 + lane) * 2 + 1] = rstd[lane];
  }
}

template <int CPB>
__global__ __launch_bounds__(256) void gn_gelu_bwd_kernel(const float* __restrict__ dact, int dstride, int L2,
                                                          const float* __restrict__ y,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          const float* __restrict__ stats, float* __restrict__ dy,
                                                          float* __restrict__ partials, int B, int L, int N) {
  constexpr int NCHK = 3 * CPB;
  constexpr int CT = NCHK * 64;
  __shared__ float red[4][3 * CT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float inv_cnt = 1.0f / (float)(L * CPB * 64);
  const int64_t tstride = (int64_t)N * CT;
  float gm[NCHK], bt[NCHK], dgm[NCHK], dbt[NCHK], dys[NCHK];
#pragma unroll
  for (int i = 0; i < NCHK; ++i) {
    gm[i] = gamma[lane + 64 * i];
    bt[i] = beta[lane + 64 * i];
    dgm[i] = 0.f;
    dbt[i] = 0.f;
    dys[i] = 0.f;
  }
  for (int64_t sidx = (int64_t)blockIdx.x * 4 + wave; sidx < (int64_t)B * N; sidx += (int64_t)gridDim.x * 4) {
    const int b = (int)(sidx / N), n = (int)(sidx - (int64_t)b * N);
    float mean[3], rstd[3];
#pragma unroll
    for (int br = 0; br < 3; ++br) {
      mean[br] = stats[(sidx * 3 + br) * 2];
      rstd[br] = stats[(sidx * 3 + br) * 2 + 1];
    }
    const float* ybase = y + ((int64_t)b * L * N + n) * CT + lane;
    const float* dbase = dact + ((int64_t)b * L2 * N + n) * CT + lane;
    float* obase = dy + ((int64_t)b * L * N + n) * CT + lane;
    float s1[3] = {0.f, 0.f, 0.f}, s2[3] = {0.f, 0.f, 0.f};
    for (int t = 0; t < L; ++t) {
      const bool has = (t % dstride) == 0;
      const float* p = ybase + t * tstride;
      const float* dp = dbase + (t / dstride) * tstride;
#pragma unroll
      for (int br = 0; br < 3; ++br)
#pragma unroll
        for (int k = 0; k < CPB; ++k) {
          const int i = br * CPB + k;
          if (has) {
            const BwdElem e = bwd_elem<Gelu::Erf>(p[64 * i], dp[64 * i], mean[br], rstd[br], gm[i], bt[i]);
            dgm[i] += e.g * e.h;
            dbt[i] += e.g;
            const float dyh = e.d();
            s1[br] += dyh;
            s2[br] += dyh * e.h;
          }
        }
    }
#pragma unroll
    for (int br = 0; br < 3; ++br) {
      s1[br] = wave_sum(s1[br]) * inv_cnt;
      s2[br] = wave_sum(s2[br]) * inv_cnt;
    }
    for (int t = 0; t < L; ++t) {
      const bool has = (t % dstride) == 0;
      const float* p = ybase + t * tstride;
      const float* dp = dbase + (t / dstride) * tstride;
      float* o = obase + t * tstride;
#pragma unroll
      for (int br = 0; br < 3; ++br)
#pragma unroll
        for (int k = 0; k < CPB; ++k) {
          const int i = br * CPB + k;
          const float yh = y_hat(p[64 * i], mean[br], rstd[br]);
          float dyh = 0.f;
          if (has) dyh = bwd_elem<Gelu::Erf>(p[64 * i], dp[64 * i], mean[br], rstd[br], gm[i], bt[i]).d();
          const float dyv = dy_elem(rstd[br], dyh, s1[br], s2[br], yh);
          o[64 * i] = dyv;
          dys[i] += dyv;                    // column sum of dy = gradient of the Conv1d bias in front of this norm
        }
    }
  }
#pragma unroll
  for (int i = 0; i < NCHK; ++i) {
    red[wave][lane + 64 * i] = dgm[i];
    red[wave][CT + lane + 64 * i] = dbt[i];
    red[wave][2 * CT + lane + 64 * i] = dys[i];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 3 * CT; c += 256)
    partials[(int64_t)blockIdx.x * 3 * CT + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}


// ------------------------------------------------------------------------------ GroupNorm(1) + GELU, register-resident
// Fast path for sequences that fit in registers: WPS waves (LPS = 64*WPS lanes) own one sequence, a lane holds
// NP <= NPMAX float4 "pairs" (t, channel quad) of it, so y (and dact) are read from HBM exactly once with
// 16-byte loads and every statistic is a register pass.  Pair j = l2 + LPS*i of lane l2 (i = 0..NP-1) is row
// t = j / QPR, quad = j % QPR (QPR = CT/4 quads per row).  3*LPS is a multiple of QPR for CT in {192, 384, 768},
// so a lane only ever meets three different channel quads (slot = i % 3): three gamma/beta quads and three
// parameter-gradient accumulators per lane.  Requires L*QPR % LPS == 0 and L*QPR/LPS <= NPMAX.
//   <WPS 4, NPMAX 9>: the default shapes (L 48 x 192 ch, L 24 x 384 ch): 9 pairs, ~150 VGPRs in the backward
//   <WPS 8, NPMAX 9>: twice the sequence length (L_in = 96), one 512-thread block per sequence
//   <WPS 2, NPMAX 18>: forward only, short sequences whose quad count is not a multiple of 256

// The input y stays fp32 where the outputs are bf16 (gn_ld4 / gn_st4): these kernels are bound by requests in flight, not
// bytes, and 8-byte loads made them 20 % slower (measured).
template <int CPB, int WPS>
struct GnGeom {
  static constexpr int CT = 192 * CPB;
  static constexpr int QPR = CT / 4;        // quads per row
  static constexpr int QPB = QPR / 3;       // quads per branch
  static constexpr int LPS = 64 * WPS;      // lanes per sequence
  static constexpr int NTHR = WPS > 4 ? 64 * WPS : 256;   // threads per block
  static constexpr int SPB = NTHR / LPS;    // sequences per block
  static constexpr int DT = LPS / QPR, DQ = LPS % QPR;
  static_assert((3 * LPS) % QPR == 0, "slot period");
};
// (The slot setup -- qs[], brs[] -- and the t / q walk below stand in both register kernels.  As members of GnGeom, by
//  reference or as a small struct, they changed how the compiler packs the backward's multiply-adds: other last bits.)

template <int CPB, int WPS, int GN_NPMAX, bool IO16>
__global__ __launch_bounds__((GnGeom<CPB, WPS>::NTHR)) void gn_gelu_fwd_reg(const void* __restrict__ y, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, void* __restrict__ act,
                                                       float* __restrict__ stats, int B, int L, int N, float eps, int NP,
                                                       int astride) {
  // astride > 1: only the time steps t % astride == 0 are written, into a COMPACT (B, ceil(L / astride), N, CT) tensor --
  // the strided 1x1 conv behind the block (modules.py:36-41) reads nothing else, while the statistics need every step
  using G = GnGeom<CPB, WPS>;
  __shared__ float xch[G::NTHR / 64][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sp = wave / WPS, half = wave % WPS, l2 = half * 64 + lane;
  int64_t sidx = (int64_t)blockIdx.x * G::SPB + sp;
  const bool live = sidx < (int64_t)B * N;
  if (!live) sidx = (int64_t)B * N - 1;                  // keep the wave in the barriers; it stores nothing
  const int b = (int)(sidx / N), n = (int)(sidx - (int64_t)b * N);
  const int64_t tstride = (int64_t)N * G::CT;
  const int64_t base = ((int64_t)b * L * N + n) * G::CT;
  const float inv_cnt = 1.0f / (float)(L * CPB * 64);

  // the lane's three channel quads
  int qs[3], brs[3];
  {
    int q = l2 % G::QPR;
#pragma unroll
    for (int s_ = 0; s_ < 3; ++s_) {
      qs[s_] = q;
      brs[s_] = q / G::QPB;
      q += G::DQ;
      if (q >= G::QPR) q -= G::QPR;
    }
  }
  float4 v[GN_NPMAX];
  int32_t off[GN_NPMAX];                                 // relative to the sequence base (host checks L*N*CT < 2^31)
  int32_t aoff[GN_NPMAX];                                // the same in the (compact) act tensor; -1: this step is not written
  const int La = (L + astride - 1) / astride;
  const int64_t abase = ((int64_t)b * La * N + n) * G::CT;
  {
    int t = l2 / G::QPR, q = l2 % G::QPR;
#pragma unroll
    for (int i = 0; i < GN_NPMAX; ++i) {
      off[i] = t * (int32_t)tstride + q * 4;
      aoff[i] = (t % astride) == 0 ? (t / astride) * (int32_t)tstride + q * 4 : -1;
      if (i < NP) v[i] = gn_ld4<false>(y, base + off[i]);      // y stays fp32: 8-byte loads make the kernel slower, not faster
      t += G::DT;
      q += G::DQ;
      if (q >= G::QPR) { q -= G::QPR; ++t; }
    }
  }
  float4 gm[3], bt[3];
#pragma unroll
  for (int s_ = 0; s_ < 3; ++s_) {
    gm[s_] = *reinterpret_cast<const float4*>(gamma + qs[s_] * 4);
    bt[s_] = *reinterpret_cast<const float4*>(beta + qs[s_] * 4);
  }
  // mean
  float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < GN_NPMAX; ++i)
    if (i < NP) acc[i % 3] += sum4(v[i]);
  float mean[3];
#pragma unroll
  for (int bb = 0; bb < 3; ++bb)
    mean[bb] = (brs[0] == bb ? acc[0] : 0.f) + (brs[1] == bb ? acc[1] : 0.f) + (brs[2] == bb ? acc[2] : 0.f);
  seq_reduce3<WPS>(mean, xch, wave, lane);
#pragma unroll
  for (int bb = 0; bb < 3; ++bb) mean[bb] *= inv_cnt;
  float ms[3];
#pragma unroll
  for (int s_ = 0; s_ < 3; ++s_) ms[s_] = sel3(brs[s_], mean[0], mean[1], mean[2]);
  // variance (two-pass form, like nn.GroupNorm)
  acc[0] = acc[1] = acc[2] = 0.f;
#pragma unroll
  for (int i = 0; i < GN_NPMAX; ++i)
    if (i < NP) {
      const float m = ms[i % 3];
      const float dx = v[i].x - m, dy_ = v[i].y - m, dz = v[i].z - m, dw = v[i].w - m;
      acc[i % 3] += (dx * dx + dy_ * dy_) + (dz * dz + dw * dw);
    }
  float rstd[3];
#pragma unroll
  for (int bb = 0; bb < 3; ++bb)
    rstd[bb] = (brs[0] == bb ? acc[0] : 0.f) + (brs[1] == bb ? acc[1] : 0.f) + (brs[2] == bb ? acc[2] : 0.f);
  seq_reduce3<WPS>(rstd, xch, wave, lane);
#pragma unroll
  for (int bb = 0; bb < 3; ++bb) rstd[bb] = 1.0f / sqrtf(rstd[bb] * inv_cnt + eps);
  float rs[3];
#pragma unroll
  for (int s_ = 0; s_ < 3; ++s_) rs[s_] = sel3(brs[s_], rstd[0], rstd[1], rstd[2]);
  if (live) {
#pragma unroll
    for (int i = 0; i < GN_NPMAX; ++i)
      if (i < NP && aoff[i] >= 0) {
        const int s_ = i % 3;
        float4 o;
        o.x = fwd_elem<Gelu::Fast>(v[i].x, ms[s_], rs[s_], gm[s_].x, bt[s_].x);
        o.y = fwd_elem<Gelu::Fast>(v[i].y, ms[s_], rs[s_], gm[s_].y, bt[s_].y);
        o.z = fwd_elem<Gelu::Fast>(v[i].z, ms[s_], rs[s_], gm[s_].z, bt[s_].z);
        o.w = fwd_elem<Gelu::Fast>(v[i].w, ms[s_], rs[s_], gm[s_].w, bt[s_].w);
        gn_st4<IO16>(act, abase + aoff[i], o);
      }
    if (half == 0 && lane < 3) {
      stats[(sidx * 3 + lane) * 2] = sel3(lane, mean[0], mean[1], mean[2]);
      stats[(sidx * 3 + lane) * 2 + 1] = sel3(lane, rstd[0], rstd[1], rstd[2]);
    }
  }
}

// Y16: y itself is bf16 (round 4; 8-byte loads: the same number of requests as the fp32 form, half the bytes -- the
// 8-channel kernels below issue a third of the requests per lane and run slower in this direction)
template <int CPB, int WPS, int GN_NPMAX, bool IO16, bool D16 = false, bool Y16 = false>
__global__ __launch_bounds__((GnGeom<CPB, WPS>::NTHR)) void gn_gelu_bwd_reg(const void* __restrict__ dact, int dstride, int L2,
                                                       const void* __restrict__ y, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ stats,
                                                       void* __restrict__ dy, float* __restrict__ partials, int B,
                                                       int L, int N, int NP) {
  using G = GnGeom<CPB, WPS>;
  __shared__ float xch[G::NTHR / 64][3];
  __shared__ float red[3 * G::CT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sp = wave / WPS, half = wave % WPS, l2 = half * 64 + lane;
  const int64_t tstride = (int64_t)N * G::CT;
  const float inv_cnt = 1.0f / (float)(L * CPB * 64);
  for (int c = threadIdx.x; c < 3 * G::CT; c += G::NTHR) red[c] = 0.f;

  int qs[3], brs[3];
  {
    int q = l2 % G::QPR;
#pragma unroll
    for (int s_ = 0; s_ < 3; ++s_) {
      qs[s_] = q;
      brs[s_] = q / G::QPB;
      q += G::DQ;
      if (q >= G::QPR) q -= G::QPR;
    }
  }
  float4 gm[3], bt[3], dgm[3], dbt[3], dys[3];
#pragma unroll
  for (int s_ = 0; s_ < 3; ++s_) {
    gm[s_] = *reinterpret_cast<const float4*>(gamma + qs[s_] * 4);
    bt[s_] = *reinterpret_cast<const float4*>(beta + qs[s_] * 4);
    dgm[s_] = dbt[s_] = dys[s_] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int64_t S = (int64_t)B * N;
  for (int64_t s0 = (int64_t)blockIdx.x * G::SPB; s0 < S; s0 += (int64_t)gridDim.x * G::SPB) {
    int64_t sidx = s0 + sp;
    const bool live = sidx < S;
    if (!live) sidx = S - 1;
    const int b = (int)(sidx / N), n = (int)(sidx - (int64_t)b * N);
    const int64_t ybase = ((int64_t)b * L * N + n) * G::CT;
    const int64_t dbase = ((int64_t)b * L2 * N + n) * G::CT;
    float mean[3], rstd[3];
#pragma unroll
    for (int bb = 0; bb < 3; ++bb) {
      mean[bb] = stats[(sidx * 3 + bb) * 2];
      rstd[bb] = stats[(sidx * 3 + bb) * 2 + 1];
    }
    float ms[3], rs[3];
#pragma unroll
    for (int s_ = 0; s_ < 3; ++s_) {
      ms[s_] = sel3(brs[s_], mean[0], mean[1], mean[2]);
      rs[s_] = sel3(brs[s_], rstd[0], rstd[1], rstd[2]);
    }
    float4 yh[GN_NPMAX], gd[GN_NPMAX];                    // y (then y_hat) and dact (then d y_hat)
    int32_t off[GN_NPMAX];
    {
      int t = l2 / G::QPR, q = l2 % G::QPR;
#pragma unroll
      for (int i = 0; i < GN_NPMAX; ++i) {
        off[i] = t * (int32_t)tstride + q * 4;
        if (i < NP) {
          yh[i] = gn_ld4<Y16>(y, ybase + off[i]);
          const bool has = (t % dstride) == 0;
          // (D16: the gradient of the strided 1x1 conv's input arrives as the bf16 tensor its bf16 GEMM wrote)
          gd[i] = has ? gn_ld4<D16>(dact, dbase + (t / dstride) * (int32_t)tstride + q * 4)
                      : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        t += G::DT;
        q += G::DQ;
        if (q >= G::QPR) { q -= G::QPR; ++t; }
      }
    }
    float a1[3] = {0.f, 0.f, 0.f}, a2[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < GN_NPMAX; ++i)
      if (i < NP) {
        const int s_ = i % 3;
        // one component: y -> y_hat and dact -> d y_hat in place, the sums of the slot.  (The macro only names the component;
        // the math is bwd_elem.  A lambda taking the components by reference compiled to other multiply-add pairings.)
#define GN_ELEM(c)                                                                                  \
  {                                                                                                 \
    const BwdElem e = bwd_elem<Gelu::Fast>(yh[i].c, gd[i].c, ms[s_], rs[s_], gm[s_].c, bt[s_].c); \
    if (live) { dgm[s_].c += e.g * e.h; dbt[s_].c += e.g; }                                         \
    const float d_ = e.d();                                                                         \
    a1[s_] += d_;                                                                                   \
    a2[s_] += d_ * e.h;                                                                             \
    yh[i].c = e.h;                                                                                  \
    gd[i].c = d_;                                                                                   \
  }
        GN_ELEM(x) GN_ELEM(y) GN_ELEM(z) GN_ELEM(w)
#undef GN_ELEM
      }
    float s1[3], s2[3];
#pragma unroll
    for (int bb = 0; bb < 3; ++bb) {
      s1[bb] = (brs[0] == bb ? a1[0] : 0.f) + (brs[1] == bb ? a1[1] : 0.f) + (brs[2] == bb ? a1[2] : 0.f);
      s2[bb] = (brs[0] == bb ? a2[0] : 0.f) + (brs[1] == bb ? a2[1] : 0.f) + (brs[2] == bb ? a2[2] : 0.f);
    }
    seq_reduce3<WPS>(s1, xch, wave, lane);
    seq_reduce3<WPS>(s2, xch, wave, lane);
    float m1[3], m2[3];
#pragma unroll
    for (int s_ = 0; s_ < 3; ++s_) {
      m1[s_] = sel3(brs[s_], s1[0], s1[1], s1[2]) * inv_cnt;
      m2[s_] = sel3(brs[s_], s2[0], s2[1], s2[2]) * inv_cnt;
    }
    if (live) {
#pragma unroll
      for (int i = 0; i < GN_NPMAX; ++i)
        if (i < NP) {
          const int s_ = i % 3;
          float4 o;
          o.x = dy_elem(rs[s_], gd[i].x, m1[s_], m2[s_], yh[i].x);
          o.y = dy_elem(rs[s_], gd[i].y, m1[s_], m2[s_], yh[i].y);
          o.z = dy_elem(rs[s_], gd[i].z, m1[s_], m2[s_], yh[i].z);
          o.w = dy_elem(rs[s_], gd[i].w, m1[s_], m2[s_], yh[i].w);
          gn_st4<IO16>(dy, ybase + off[i], o);
          dys[s_].x += o.x; dys[s_].y += o.y; dys[s_].z += o.z; dys[s_].w += o.w;   // conv-bias gradient
        }
    }
  }
  // block reduction of the per-lane parameter gradients (each channel quad is held by NTHR*3/QPR (lane, slot) pairs)
  // -> one partial row.  In a FIXED order, so that the gradients repeat bit for bit: for a given slot the holders of
  // one quad are the lanes with the same l2 % QPR, ranked by (sequence of the block, l2 / QPR); in round (slot, rank)
  // every quad has at most one writer, which adds with a plain read-modify-write.  (LDS float atomics here made
  // d gamma / d beta / d conv-bias order-dependent in the last bits.)
  {
    constexpr int RMAX = (G::LPS + G::QPR - 1) / G::QPR;
    const int rank = sp * RMAX + l2 / G::QPR;
#pragma unroll
    for (int s_ = 0; s_ < 3; ++s_) {
      const int c = qs[s_] * 4;
      for (int r = 0; r < G::SPB * RMAX; ++r) {
        __syncthreads();
        if (r == rank) {
          red[c + 0] += dgm[s_].x; red[c + 1] += dgm[s_].y; red[c + 2] += dgm[s_].z; red[c + 3] += dgm[s_].w;
          red[G::CT + c + 0] += dbt[s_].x; red[G::CT + c + 1] += dbt[s_].y;
          red[G::CT + c + 2] += dbt[s_].z; red[G::CT + c + 3] += dbt[s_].w;
          red[2 * G::CT + c + 0] += dys[s_].x; red[2 * G::CT + c + 1] += dys[s_].y;
          red[2 * G::CT + c + 2] += dys[s_].z; red[2 * G::CT + c + 3] += dys[s_].w;
        }
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 3 * G::CT; c += G::NTHR) partials[(int64_t)blockIdx.x * 3 * G::CT + c] = red[c];
}

// ------------------------------------------------------------------------------ GroupNorm(1) + GELU on a bf16 y (round 4)
// bf16 mode: the conv output y is the bf16 tensor a bf16 Conv1d hands to the fp32 GroupNorm under autocast (train.py:68;
// conv_fwd_seq writes it as such), and every tensor these kernels touch is bf16 (y, act, dact, dy).  The register-resident
// kernels above are bound by memory requests in flight, not bytes -- fed 8-byte quads they got slower, not faster -- so here
// a lane's unit is an OCT (8 consecutive channels = one 16-byte load / store): the same number of requests per lane, twice
// the elements.  (Geometry: GnGeom8 below.)  The sequence need not fill the last round of lanes: rows past L are skipped.
// Geometry: SIX waves (384 lanes) own one sequence and a lane keeps ONE channel oct for the whole kernel (384 is a multiple
// of OPR = 24, 48, 96): lane l2 holds oct l2 % OPR of the rows t = l2 / OPR + k * (384 / OPR), k < NG.  One gamma / beta oct
// and one set of parameter-gradient accumulators per lane (the three-slot form of the fp32-y kernels needs 72 + 48
// registers for them at 8 channels per unit and ran at one wave per SIMD).
template <int CPB>
struct GnGeom8 {
  static constexpr int CT = 192 * CPB;
  static constexpr int OPR = CT / 8;        // octs per row
  static constexpr int OPB = OPR / 3;       // octs per branch
  static constexpr int LPS = 384;           // lanes per sequence = threads per block
  static constexpr int DT = LPS / OPR;      // rows between a lane's consecutive octs
  static_assert(LPS % OPR == 0, "a lane keeps its channel oct");
};

template <int CPB, int NG>
__global__ __launch_bounds__(384) void gn_gelu_fwd_reg16(const void* __restrict__ y, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, void* __restrict__ act,
                                                         float* __restrict__ stats, int B, int L, int N, float eps,
                                                         int astride) {
  using G = GnGeom8<CPB>;
  __shared__ float xch[6][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l2 = threadIdx.x;
  const int64_t sidx = blockIdx.x;                        // one sequence per block
  const int b = (int)(sidx / N), n = (int)(sidx - (int64_t)b * N);
  const int64_t tstride = (int64_t)N * G::CT;
  const int64_t base = ((int64_t)b * L * N + n) * G::CT;
  const int La = (L + astride - 1) / astride;
  const int64_t abase = ((int64_t)b * La * N + n) * G::CT;
  const float inv_cnt = 1.0f / (float)(L * CPB * 64);
  const int q = l2 % G::OPR, t0 = l2 / G::OPR, br = q / G::OPB;
  f32x8 v[NG];
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    const int t = t0 + k * G::DT;
    const int tc = t < L ? t : L - 1;                      // clamped: an unconditional load, the value is not used
    v[k] = gn_ld8(y, base + tc * (int32_t)tstride + q * 8);
    if (t >= L)
#pragma unroll
      for (int e = 0; e < 8; ++e) v[k][e] = 0.f;
  }
  const f32x8 gm = gn_ld8f(gamma + q * 8), bt = gn_ld8f(beta + q * 8);
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < NG; ++k) acc += sum8(v[k]);          // absent octs hold zeros
  float mean[3] = {br == 0 ? acc : 0.f, br == 1 ? acc : 0.f, br == 2 ? acc : 0.f};
  seq_reduce3<6>(mean, xch, wave, lane);
#pragma unroll
  for (int bb = 0; bb < 3; ++bb) mean[bb] *= inv_cnt;
  const float m = sel3(br, mean[0], mean[1], mean[2]);
  acc = 0.f;
#pragma unroll
  for (int k = 0; k < NG; ++k)
    if (t0 + k * G::DT < L) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[k][e] - m;
        acc += d * d;
      }
    }
  float rstd[3] = {br == 0 ? acc : 0.f, br == 1 ? acc : 0.f, br == 2 ? acc : 0.f};
  seq_reduce3<6>(rstd, xch, wave, lane);
#pragma unroll
  for (int bb = 0; bb < 3; ++bb) rstd[bb] = 1.0f / sqrtf(rstd[bb] * inv_cnt + eps);
  const float rs = sel3(br, rstd[0], rstd[1], rstd[2]);
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    const int t = t0 + k * G::DT;
    if (t < L && (t % astride) == 0) {
      f32x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = fwd_elem<Gelu::Fast>(v[k][e], m, rs, gm[e], bt[e]);
      gn_st8(act, abase + (t / astride) * (int32_t)tstride + q * 8, o);
    }
  }
  if (l2 < 3) {
    stats[(sidx * 3 + l2) * 2] = sel3(l2, mean[0], mean[1], mean[2]);
    stats[(sidx * 3 + l2) * 2 + 1] = sel3(l2, rstd[0], rstd[1], rstd[2]);
  }
}

template <int CPB, int NG>
#ifndef GN16_OCC
#define GN16_OCC 3       // waves per SIMD the 3-oct backward is compiled for (168 registers, ~8 spilled; 2 = 176, none)
#endif
__global__ __launch_bounds__(384, (NG == 3 ? GN16_OCC : 2)) void gn_gelu_bwd_reg16(const void* __restrict__ dact, int dstride, int L2,
                                                         const void* __restrict__ y, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ stats,
                                                         void* __restrict__ dy, float* __restrict__ partials, int B,
                                                         int L, int N) {
  using G = GnGeom8<CPB>;
  __shared__ float xch[6][3];
  __shared__ float red[3 * G::CT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l2 = threadIdx.x;
  const int64_t tstride = (int64_t)N * G::CT;
  const float inv_cnt = 1.0f / (float)(L * CPB * 64);
  const int q = l2 % G::OPR, t0 = l2 / G::OPR, br = q / G::OPB;
  const f32x8 gm = gn_ld8f(gamma + q * 8), bt = gn_ld8f(beta + q * 8);
  f32x8 dgm, dbt, dys;
#pragma unroll
  for (int e = 0; e < 8; ++e) dgm[e] = dbt[e] = dys[e] = 0.f;
  const int64_t S = (int64_t)B * N;
  for (int64_t sidx = blockIdx.x; sidx < S; sidx += gridDim.x) {
    const int b = (int)(sidx / N), n = (int)(sidx - (int64_t)b * N);
    const int64_t ybase = ((int64_t)b * L * N + n) * G::CT;
    const int64_t dbase = ((int64_t)b * L2 * N + n) * G::CT;
    const float m = stats[(sidx * 3 + br) * 2], rs = stats[(sidx * 3 + br) * 2 + 1];
    f32x8 yh[NG], gd[NG];
#pragma unroll
    for (int k = 0; k < NG; ++k) {
      const int t = t0 + k * G::DT;
      const int tc = t < L ? t : L - 1;
      yh[k] = gn_ld8(y, ybase + tc * (int32_t)tstride + q * 8);
      gd[k] = gn_ld8(dact, dbase + (tc / dstride) * (int32_t)tstride + q * 8);     // unconditional (clamped), masked below
      if (t >= L || (tc % dstride) != 0)
#pragma unroll
        for (int e = 0; e < 8; ++e) gd[k][e] = 0.f;
    }
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
      const bool has = t0 + k * G::DT < L;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const BwdElem r = bwd_elem<Gelu::Fast>(yh[k][e], gd[k][e], m, rs, gm[e], bt[e]);   // gd = 0 where there is no gradient
        dgm[e] += r.g * r.h;
        dbt[e] += r.g;
        const float d_ = r.d();
        a1 += d_;
        a2 += d_ * r.h;
        yh[k][e] = has ? r.h : 0.f;
        gd[k][e] = d_;
      }
    }
    float s1[3] = {br == 0 ? a1 : 0.f, br == 1 ? a1 : 0.f, br == 2 ? a1 : 0.f};
    float s2[3] = {br == 0 ? a2 : 0.f, br == 1 ? a2 : 0.f, br == 2 ? a2 : 0.f};
    seq_reduce3<6>(s1, xch, wave, lane);
    seq_reduce3<6>(s2, xch, wave, lane);
    const float m1 = sel3(br, s1[0], s1[1], s1[2]) * inv_cnt, m2 = sel3(br, s2[0], s2[1], s2[2]) * inv_cnt;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
      const int t = t0 + k * G::DT;
      if (t < L) {
        f32x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          o[e] = dy_elem(rs, gd[k][e], m1, m2, yh[k][e]);
          dys[e] += o[e];                                  // conv-bias gradient
        }
        gn_st8(dy, ybase + t * (int32_t)tstride + q * 8, o);
      }
    }
  }
  // block reduction in a FIXED order: the holders of one oct are the lanes l2 = q + OPR * j, j = 0 .. DT-1, taken in turn
  for (int c = threadIdx.x; c < 3 * G::CT; c += 384) red[c] = 0.f;
  for (int j = 0; j < G::DT; ++j) {
    __syncthreads();
    if (t0 == j) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[q * 8 + e] += dgm[e];
        red[G::CT + q * 8 + e] += dbt[e];
        red[2 * G::CT + q * 8 + e] += dys[e];
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 3 * G::CT; c += 384) partials[(int64_t)blockIdx.x * 3 * G::CT + c] = red[c];
}

// GroupNorm(1) + GELU forward with the statistics GIVEN (conv_fwd_seq computes them from the y it holds in registers): what is
// left is elementwise and needs only the time steps the strided 1x1 conv reads -- one oct (8 channels) per lane per visit,
// every access a 16-byte one, no sequence held anywhere, no synchronisation.  act is the compact (B, L / stride, N, CT) tensor.
__global__ __launch_bounds__(256) void gn_apply_fwd16_kernel(const void* __restrict__ y, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, void* __restrict__ act,
                                                             const float* __restrict__ stats, int B, int L, int N, int Cout,
                                                             int stride) {
  const int CT = 3 * Cout, OPR = CT / 8;                       // octs per row
  const int Lo = (L + stride - 1) / stride;
  const int64_t total = (int64_t)B * Lo * N * OPR;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int o = (int)(i % OPR);
    const int64_t row = i / OPR;                               // (b, to, n)
    const int n = (int)(row % N);
    const int64_t bt = row / N;
    const int to = (int)(bt % Lo), b = (int)(bt / Lo);
    const int c = o * 8, br = c / Cout;
    const float2 ms = *reinterpret_cast<const float2*>(stats + (((int64_t)b * N + n) * 3 + br) * 2);
    const f32x8 v = gn_ld8(y, (((int64_t)b * L + (int64_t)to * stride) * N + n) * CT + c);
    const f32x8 g = gn_ld8f(gamma + c), be = gn_ld8f(beta + c);
    f32x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = fwd_elem<Gelu::Fast>(v[e], ms.x, ms.y, g[e], be[e]);
    gn_st8(act, row * CT + c, r);
  }
}

// ------------------------------------------------------------------ GroupNorm(1) + GELU backward on bf16 tensors, split (round 4)
// The sequence-resident backward (a block holds one sequence in registers: load, reduce, barrier, reduce, barrier, write)
// runs at 2.3 TB/s of its 1.07 GB -- two waves per SIMD, every phase exposed.  The same arithmetic as TWO streaming kernels
// with no resident sequence:
//   sums   a block owns NPB nodes of one sample and walks the time steps the strided 1x1 conv read (the only ones with a
//          gradient); a lane keeps one (node, channel oct): sum d and sum d * y_hat per (sequence, branch), d gamma / d beta
//          per channel in registers across the block's items.  Reads y (those steps) + dact: 0.43 GB.
//   apply  elementwise: dy = rstd * (d - mean(d) - y_hat * mean(d y_hat)), d recomputed (GELU' a second time is cheaper than
//          a resident sequence); a lane keeps its channel oct, so the conv-bias gradient (column sums of dy) stays in
//          registers.  Reads y + dact, writes dy: 1.07 GB.
// Both deterministic (fixed lane -> channel map, per-block partial rows summed by tecm_colsum).
template <int CPB>
__global__ __launch_bounds__(256, 4) void gn_bwd_sums16_kernel(const void* __restrict__ dact, int dstride, int L2,
                                                            const void* __restrict__ y, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ stats,
                                                            float* __restrict__ sums, float* __restrict__ partials, int B,
                                                            int L, int N, int active) {
  constexpr int CT = 192 * CPB, OPR = CT / 8, OPB = OPR / 3, NPB = 256 / OPR;
  __shared__ float red[NPB][OPR][2];
  __shared__ float pg[2][NPB][CT];
  const int nl = threadIdx.x / OPR, o = threadIdx.x - nl * OPR;
  const bool lane_on = nl < NPB;
  const int c = o * 8, br = o / OPB;
  const f32x8 gm = lane_on ? gn_ld8f(gamma + c) : f32x8{}, bt = lane_on ? gn_ld8f(beta + c) : f32x8{};
  f32x8 dg = {}, db = {};
  const int nblk = (N + NPB - 1) / NPB;
  const int items = B * nblk;
  // `active` blocks share the items evenly (the rest of the grid only writes its zero partial row)
  for (int item = blockIdx.x < active ? blockIdx.x : items; item < items; item += active) {
    const int b = item / nblk, n = (item - b * nblk) * NPB + nl;
    const bool on = lane_on && n < N;
    const int nn = on ? n : 0;
    const float2 ms = *reinterpret_cast<const float2*>(stats + (((int64_t)b * N + nn) * 3 + (lane_on ? br : 0)) * 2);
    float a1 = 0.f, a2 = 0.f;
    if (on) {
      const int64_t yb = ((int64_t)b * L * N + nn) * CT + c, dbs = ((int64_t)b * L2 * N + nn) * CT + c;
      const int64_t ystep = (int64_t)dstride * N * CT, dstep = (int64_t)N * CT;
#pragma unroll 4
      for (int t2 = 0; t2 < L2; ++t2) {
        const f32x8 yv = gn_ld8(y, yb + t2 * ystep), dv = gn_ld8(dact, dbs + t2 * dstep);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const BwdElem r = bwd_elem<Gelu::Fast>(yv[e], dv[e], ms.x, ms.y, gm[e], bt[e]);
          dg[e] += r.g * r.h;
          db[e] += r.g;
          const float d_ = r.d();
          a1 += d_;
          a2 += d_ * r.h;
        }
      }
    }
    __syncthreads();                                          // red is free again
    if (lane_on) { red[nl][o][0] = a1; red[nl][o][1] = a2; }
    __syncthreads();
    if (threadIdx.x < NPB * 3) {                              // (node, branch): OPB octs in a fixed order
      const int q = threadIdx.x / 3, bb = threadIdx.x - q * 3;
      const int n2 = (item - b * nblk) * NPB + q;
      float t1 = 0.f, t2 = 0.f;
      for (int k = 0; k < OPB; ++k) { t1 += red[q][bb * OPB + k][0]; t2 += red[q][bb * OPB + k][1]; }
      if (n2 < N) {
        float* so = sums + (((int64_t)b * N + n2) * 3 + bb) * 2;
        so[0] = t1;
        so[1] = t2;
      }
    }
  }
  __syncthreads();
  if (lane_on) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { pg[0][nl][c + e] = dg[e]; pg[1][nl][c + e] = db[e]; }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 2 * CT; k += 256) {
    const int w = k / CT, cc = k - w * CT;
    float t = 0.f;
    for (int q = 0; q < NPB; ++q) t += pg[w][q][cc];
    partials[(int64_t)blockIdx.x * 3 * CT + k] = t;
  }
}

template <int CPB>
__global__ __launch_bounds__(256) void gn_bwd_apply16_kernel(const void* __restrict__ dact, int dstride, int L2,
                                                             const void* __restrict__ y, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ stats,
                                                             const float* __restrict__ sums, void* __restrict__ dy,
                                                             float* __restrict__ partials, int B, int L, int N) {
  constexpr int CT = 192 * CPB, OPR = CT / 8, OPB = OPR / 3, RPB = 256 / OPR;
  __shared__ float pg[RPB][CT];
  const int rl = threadIdx.x / OPR, o = threadIdx.x - rl * OPR;
  const bool lane_on = rl < RPB;
  const int c = o * 8, br = o / OPB;
  const f32x8 gm = lane_on ? gn_ld8f(gamma + c) : f32x8{}, bt = lane_on ? gn_ld8f(beta + c) : f32x8{};
  const float inv_cnt = 1.0f / (float)(L * CPB * 64);
  f32x8 dys = {};
  const int64_t rows = (int64_t)B * L * N;
  if (lane_on)
    for (int64_t row = (int64_t)blockIdx.x * RPB + rl; row < rows; row += (int64_t)gridDim.x * RPB) {
      const int n = (int)(row % N);
      const int64_t bt_ = row / N;
      const int t = (int)(bt_ % L), b = (int)(bt_ / L);
      const int64_t si = (((int64_t)b * N + n) * 3 + br) * 2;
      const float2 ms = *reinterpret_cast<const float2*>(stats + si);
      const float2 sm = *reinterpret_cast<const float2*>(sums + si);
      const float m1 = sm.x * inv_cnt, m2 = sm.y * inv_cnt;
      const f32x8 yv = gn_ld8(y, row * CT + c);
      const bool has = (t % dstride) == 0;
      f32x8 dv = {};
      if (has) dv = gn_ld8(dact, (((int64_t)b * L2 + t / dstride) * N + n) * CT + c);
      f32x8 ov;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float h_ = y_hat(yv[e], ms.x, ms.y);
        const float d_ = has ? bwd_elem<Gelu::Fast>(yv[e], dv[e], ms.x, ms.y, gm[e], bt[e]).d() : 0.f;
        ov[e] = dy_elem(ms.y, d_, m1, m2, h_);
        dys[e] += ov[e];
      }
      gn_st8(dy, row * CT + c, ov);
    }
  if (lane_on) {
#pragma unroll
    for (int e = 0; e < 8; ++e) pg[rl][c + e] = dys[e];
  }
  __syncthreads();
  for (int k = threadIdx.x; k < CT; k += 256) {
    float t = 0.f;
    for (int q = 0; q < RPB; ++q) t += pg[q][k];
    partials[(int64_t)blockIdx.x * 3 * CT + 2 * CT + k] = t;
  }
}

// ------------------------------------------------------------------------------ routing: which kernel serves a call
// Decided here and nowhere else: the launchers, tecm_gn_reg_supported / tecm_gn_y16_supported and tecm_gn_fwd_path /
// tecm_gn_bwd_path all ask gn_fwd_plan / gn_bwd_plan.
int gn_blocks(int64_t S) {
  const int64_t want = (S + 3) / 4;
  return (int)(want < 1024 ? want : 1024);
}
// pairs per lane of the register-resident GroupNorm path with `wps` waves per sequence, 0 when the sequence does
// not fit / is not 16-byte friendly
int gn_reg_pairs(int L, int N, int Cout, int wps, int npmax, const void* a, const void* b) {
  const int64_t quads = (int64_t)L * (3 * Cout / 4);
  const int lps = 64 * wps;
  if ((int64_t)L * N * 3 * Cout >= (1ll << 31)) return 0;      // 32-bit offsets inside one sample
  if (quads % lps != 0 || quads / lps > npmax) return 0;
  if (!tecm_aligned(a, 16) || !tecm_aligned(b, 16)) return 0;
  return (int)(quads / lps);
}
// octs per lane of the all-bf16 kernels (3 or 6; 384 lanes per sequence), 0 when the sequence does not fit
int gn16_ng(int L, int N, int Cout, const void* a, const void* b) {
  if (Cout != 64 && Cout != 128 && Cout != 256) return 0;
  const int64_t octs = (int64_t)L * (3 * Cout / 8);
  if ((int64_t)L * N * 3 * Cout >= (1ll << 31)) return 0;
  if ((a && !tecm_aligned(a, 16)) || (b && !tecm_aligned(b, 16))) return 0;
  if (octs <= 384 * 3) return 3;
  if (octs <= 384 * 6) return 6;
  return 0;
}

// GN_ROWS: gn_gelu_{fwd,bwd}_kernel<CPB> (generic, multi-pass, fp32 tensors only); GN_REG: gn_gelu_{fwd,bwd}_reg<CPB, WPS, NPMAX, ...>
// (register-resident, a quad per unit); GN_REG16: gn_gelu_{fwd,bwd}_reg16<CPB, NG> (every tensor bf16, an oct per unit);
// GN_APPLY16: gn_apply_fwd16_kernel (statistics given); GN_SPLIT16: gn_bwd_sums16_kernel<CPB> + gn_bwd_apply16_kernel<CPB>
enum GnKernel { GN_NONE, GN_ROWS, GN_REG, GN_REG16, GN_APPLY16, GN_SPLIT16 };
struct GnPlan {
  GnKernel kernel = GN_NONE;                     // GN_NONE: refused
  int cpb = 0, nthr = 0;                         // Cout / 64 (GN_APPLY16: not a template argument, 0), block size
  int wps = 0, npmax = 0, np = 0;                // GN_REG: waves per sequence, pairs per lane at most and in this call
  int ng = 0;                                    // GN_REG16: octs per lane
  bool io16 = false, d16 = false, y16 = false;   // act / dy, dact, y are bf16
  const char* why = "";                          // GN_NONE: what the launcher reports
};
GnPlan gn_refuse(const char* why) { GnPlan p; p.why = why; return p; }
GnPlan gn_pick(GnPlan p, GnKernel kernel, int nthr) { p.kernel = kernel; p.nthr = nthr; return p; }
// the register-resident geometry of `wps` waves per sequence, where it serves the sequence
bool gn_try_reg(GnPlan& p, int L, int N, int Cout, int wps, int npmax, const void* a, const void* b) {
  const int np = gn_reg_pairs(L, N, Cout, wps, npmax, a, b);
  if (np > 0) { p = gn_pick(p, GN_REG, wps > 4 ? 64 * wps : 256); p.wps = wps; p.npmax = npmax; p.np = np; }
  return np > 0;
}

GnPlan gn_fwd_plan(int B, int L, int N, int Cout, int io_bf16, int act_stride, const void* y, const void* act) {
  if (!(io_bf16 == 0 || io_bf16 == TECM_GN_OUT_BF16 || io_bf16 == (TECM_GN_OUT_BF16 | TECM_GN_Y_BF16) ||
        io_bf16 == (TECM_GN_OUT_BF16 | TECM_GN_Y_BF16 | TECM_GN_STATS_GIVEN)))
    return gn_refuse("io_bf16 is 0, OUT_BF16, OUT_BF16 | Y_BF16 or the latter | STATS_GIVEN");
  if (act_stride < 1) return gn_refuse("act_stride must be at least 1");
  GnPlan p;
  p.io16 = (io_bf16 & TECM_GN_OUT_BF16) != 0;
  p.y16 = (io_bf16 & TECM_GN_Y_BF16) != 0;
  if (io_bf16 & TECM_GN_STATS_GIVEN) {                   // elementwise: the statistics were computed by tecm_conv_fwd_bf16
    if (!(B > 0 && L > 0 && N > 0 && Cout > 0 && Cout % 8 == 0 && tecm_aligned(y, 16) && tecm_aligned(act, 16)))
      return gn_refuse("the elementwise form needs Cout % 8 == 0 and 16-byte aligned tensors");
    return gn_pick(p, GN_APPLY16, 256);
  }
  if (!(B > 0 && L > 0 && N > 0)) return gn_refuse("bad shape");
  if (p.y16) {                                           // every tensor bf16: the oct kernels
    p.ng = gn16_ng(L, N, Cout, y, act);
    if (p.ng == 0) return gn_refuse("a bf16 y needs L * 3*Cout/8 <= 2304 and Cout in {64, 128, 256}");
    p.cpb = Cout / 64;
    return gn_pick(p, GN_REG16, 384);
  }
  if (Cout != 64 && Cout != 128 && Cout != 256) return gn_refuse("Cout must be 64, 128 or 256");
  p.cpb = Cout / 64;
  // register-resident paths: one HBM read of y, float4 accesses
  if (gn_try_reg(p, L, N, Cout, 4, 9, y, act) || gn_try_reg(p, L, N, Cout, 8, 9, y, act) || gn_try_reg(p, L, N, Cout, 2, 18, y, act))
    return p;
  if (p.io16 || act_stride != 1)
    return gn_refuse("bf16 tensors and a compact strided act are served by the register-resident kernels only (L * Cout too large)");
  return gn_pick(p, GN_ROWS, 256);
}

// what tecm_groupnorm_gelu_bwd refuses before its query mode answers; nullptr: the arguments are fine
const char* gn_bwd_bad_args(int B, int L, int N, int Cout, int dstride, int io_bf16) {
  if (!((io_bf16 & ~(TECM_GN_OUT_BF16 | TECM_GN_DACT_BF16 | TECM_GN_Y_BF16)) == 0 &&
        (!(io_bf16 & TECM_GN_DACT_BF16) || (io_bf16 & TECM_GN_OUT_BF16)) &&
        (!(io_bf16 & TECM_GN_Y_BF16) || (io_bf16 & (TECM_GN_OUT_BF16 | TECM_GN_DACT_BF16)) == (TECM_GN_OUT_BF16 | TECM_GN_DACT_BF16))))
    return "io_bf16 is 0, OUT_BF16, OUT_BF16 | DACT_BF16 or all three with Y_BF16";
  if (!(B > 0 && L > 0 && N > 0 && dstride > 0)) return "bad shape";
  if (Cout != 64 && Cout != 128 && Cout != 256) return "Cout must be 64, 128 or 256";
  return nullptr;
}
GnPlan gn_bwd_plan(int B, int L, int N, int Cout, int dstride, int io_bf16, bool has_seq_sums, const void* dact, const void* y,
                   const void* dy) {
  if (const char* bad = gn_bwd_bad_args(B, L, N, Cout, dstride, io_bf16)) return gn_refuse(bad);
  GnPlan p;
  p.cpb = Cout / 64;
  p.io16 = (io_bf16 & TECM_GN_OUT_BF16) != 0;
  p.d16 = (io_bf16 & TECM_GN_DACT_BF16) != 0;
  p.y16 = (io_bf16 & TECM_GN_Y_BF16) != 0;
  if (p.y16 && has_seq_sums && (Cout == 64 || Cout == 128) && tecm_aligned(dact, 16) && tecm_aligned(y, 16) && tecm_aligned(dy, 16)) {
    // every tensor bf16 and a workspace for the per-sequence sums: the two streaming kernels (see gn_bwd_sums16_kernel)
    const char* sp = std::getenv("TECM_GN_BWD_SPLIT");
    if (!(sp && sp[0] == '0')) return gn_pick(p, GN_SPLIT16, 256);
  }
  if (p.y16) {                                           // every tensor bf16
    // the four-channel register kernel with 8-byte y / dact loads where its geometry serves the sequence (measured at B = 8:
    // 1.3x faster than the 8-channel kernel in this direction: more requests in flight per lane), else the 8-channel one
    const char* wps_env = std::getenv("TECM_GN_BWD_WPS");        // "8": force the 8-wave geometry (A/B diagnostics)
    const bool skip4 = wps_env && wps_env[0] == '8';
    if (tecm_aligned(dact, 8) && ((!skip4 && gn_try_reg(p, L, N, Cout, 4, 9, y, dy)) || gn_try_reg(p, L, N, Cout, 8, 9, y, dy))) return p;
    p.ng = gn16_ng(L, N, Cout, y, dy);
    if (p.ng == 0 || !tecm_aligned(dact, 16))
      return gn_refuse("a bf16 y needs L * 3*Cout/8 <= 2304, Cout in {64, 128, 256}, 16-byte aligned tensors");
    return gn_pick(p, GN_REG16, 384);
  }
  if (tecm_aligned(dact, 16) && (gn_try_reg(p, L, N, Cout, 4, 9, y, dy) || gn_try_reg(p, L, N, Cout, 8, 9, y, dy))) return p;
  if (p.io16 || p.d16) return gn_refuse("bf16 tensors are served by the register-resident kernels only (L * Cout too large)");
  return gn_pick(p, GN_ROWS, 256);
}

// the kernel(s) of a plan with their template arguments; "" for a refused call
const char* gn_plan_name(const GnPlan& p, const char* dir) {
  static thread_local char buf[96];
  const auto tf = [](bool b) { return b ? "true" : "false"; };
  buf[0] = 0;
  if (p.kernel == GN_ROWS) std::snprintf(buf, sizeof buf, "gn_gelu_%s_kernel<%d>", dir, p.cpb);
  else if (p.kernel == GN_REG && dir[0] == 'f')
    std::snprintf(buf, sizeof buf, "gn_gelu_fwd_reg<%d,%d,%d,%s>", p.cpb, p.wps, p.npmax, tf(p.io16));
  else if (p.kernel == GN_REG)
    std::snprintf(buf, sizeof buf, "gn_gelu_bwd_reg<%d,%d,%d,%s,%s,%s>", p.cpb, p.wps, p.npmax, tf(p.io16), tf(p.d16), tf(p.y16));
  else if (p.kernel == GN_REG16) std::snprintf(buf, sizeof buf, "gn_gelu_%s_reg16<%d,%d>", dir, p.cpb, p.ng);
  else if (p.kernel == GN_APPLY16) std::snprintf(buf, sizeof buf, "gn_apply_fwd16_kernel");
  else if (p.kernel == GN_SPLIT16) std::snprintf(buf, sizeof buf, "gn_bwd_sums16_kernel<%d>+gn_bwd_apply16_kernel<%d>", p.cpb, p.cpb);
  return buf;
}

// Cout / 64 as a compile-time constant, once per launch: f(std::integral_constant<int, CPB>)
template <class F>
void with_cpb(int cpb, F&& f) {
  if (cpb == 1) f(std::integral_constant<int, 1>{});
  else if (cpb == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 4>{});
}

}  // namespace

// 1 when BOTH directions have a register-resident kernel that takes bf16 act / dy (4 or 8 waves per sequence, at most 9 quads
// per lane; the 2-wave geometry is forward only), else 0
extern "C" int tecm_gn_reg_supported(int32_t L, int32_t N, int32_t Cout) {
  return gn_fwd_plan(1, L, N, Cout, TECM_GN_OUT_BF16, 1, nullptr, nullptr).kernel == GN_REG &&
                 gn_bwd_plan(1, L, N, Cout, 1, TECM_GN_OUT_BF16, false, nullptr, nullptr, nullptr).kernel == GN_REG
             ? 1 : 0;
}

// 1 when the all-bf16 GroupNorm kernels (TECM_GN_Y_BF16) serve sequences of L steps x 3*Cout channels, else 0
extern "C" int tecm_gn_y16_supported(int32_t L, int32_t N, int32_t Cout) {
  return gn_fwd_plan(1, L, N, Cout, TECM_GN_OUT_BF16 | TECM_GN_Y_BF16, 1, nullptr, nullptr).kernel == GN_REG16 ? 1 : 0;
}

// The kernel a call with 16-byte aligned tensors launches, template arguments included ("" where the launcher refuses).
// Pure host functions; the string lives until this thread's next call of either.
extern "C" const char* tecm_gn_fwd_path(int32_t L, int32_t N, int32_t Cout, int32_t io_bf16, int32_t act_stride) {
  return gn_plan_name(gn_fwd_plan(1, L, N, Cout, io_bf16, act_stride, nullptr, nullptr), "fwd");
}
extern "C" const char* tecm_gn_bwd_path(int32_t L, int32_t N, int32_t Cout, int32_t io_bf16, int32_t has_seq_sums) {
  return gn_plan_name(gn_bwd_plan(1, L, N, Cout, 1, io_bf16, has_seq_sums != 0, nullptr, nullptr, nullptr), "bwd");
}

extern "C" int tecm_groupnorm_gelu_fwd(const void* y_, const float* gamma, const float* beta, void* act_,
                                       float* stats, int32_t B, int32_t L, int32_t N, int32_t Cout, float eps,
                                       int32_t io_bf16, int32_t act_stride, void* stream) {
  const GnPlan p = gn_fwd_plan(B, L, N, Cout, io_bf16, act_stride, y_, act_);
  TECM_REQUIRE(p.kernel != GN_NONE, TECM_E_ARG, "tecm_groupnorm_gelu_fwd: %s (got L = %d, Cout = %d)", p.why, L, Cout);
  TECM_REQUIRE(y_ && gamma && beta && act_ && stats, TECM_E_ARG, "tecm_groupnorm_gelu_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t S = (int64_t)B * N;
  if (p.kernel == GN_APPLY16) {
    TECM_REQUIRE(tecm_aligned(gamma, 16) && tecm_aligned(beta, 16) && tecm_aligned(stats, 8), TECM_E_ARG,
                 "tecm_groupnorm_gelu_fwd: the elementwise form needs 16-byte aligned gamma / beta and 8-byte aligned stats");
    const int64_t octs = (int64_t)B * ((L + act_stride - 1) / act_stride) * N * (3 * Cout / 8);
    const int64_t want = (octs + 255) / 256;
    hipLaunchKernelGGL(gn_apply_fwd16_kernel, dim3((unsigned)(want < 16384 ? want : 16384)), dim3(256), 0, st, y_, gamma, beta, act_,
                       stats, B, L, N, Cout, (int)act_stride);
  } else {
    with_cpb(p.cpb, [&](auto cpb) {
      constexpr int CPB = decltype(cpb)::value;
      // the register kernels: one block per sequence (two sequences per block at 2 waves each)
      auto go = [&](auto kern, int64_t blocks, auto... tail) {
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(p.nthr), 0, st, y_, gamma, beta, act_, stats, B, L, N, eps, tail...,
                           (int)act_stride);
      };
      if (p.kernel == GN_REG16) {
        if (p.ng == 3) go(gn_gelu_fwd_reg16<CPB, 3>, S); else go(gn_gelu_fwd_reg16<CPB, 6>, S);
      } else if (p.kernel == GN_REG && p.wps == 4) {
        if (p.io16) go(gn_gelu_fwd_reg<CPB, 4, 9, true>, S, p.np); else go(gn_gelu_fwd_reg<CPB, 4, 9, false>, S, p.np);
      } else if (p.kernel == GN_REG && p.wps == 8) {
        if (p.io16) go(gn_gelu_fwd_reg<CPB, 8, 9, true>, S, p.np); else go(gn_gelu_fwd_reg<CPB, 8, 9, false>, S, p.np);
      } else if (p.kernel == GN_REG) {
        if (p.io16) go(gn_gelu_fwd_reg<CPB, 2, 18, true>, (S + 1) / 2, p.np); else go(gn_gelu_fwd_reg<CPB, 2, 18, false>, (S + 1) / 2, p.np);
      } else {
        hipLaunchKernelGGL(gn_gelu_fwd_kernel<CPB>, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, st, reinterpret_cast<const float*>(y_),
                           gamma, beta, reinterpret_cast<float*>(act_), stats, B, L, N, eps);
      }
    });
  }
  TECM_CHECK_LAUNCH(gn_plan_name(p, "fwd"));
  return TECM_OK;
}

extern "C" int tecm_groupnorm_gelu_bwd(const void* dact_, int32_t dstride, const void* y_, const float* gamma,
                                       const float* beta, const float* stats, void* dy_, float* dgb_partials,
                                       int32_t* num_blocks, int32_t B, int32_t L, int32_t N, int32_t Cout,
                                       int32_t io_bf16, float* seq_sums, void* stream) {
  const char* bad = gn_bwd_bad_args(B, L, N, Cout, dstride, io_bf16);
  TECM_REQUIRE(!bad, TECM_E_ARG, "tecm_groupnorm_gelu_bwd: %s (got L = %d, Cout = %d)", bad, L, Cout);
  const int nb = gn_blocks((int64_t)B * N);
  if (num_blocks) *num_blocks = nb;
  if (dy_ == nullptr) return TECM_OK;   // query mode
  TECM_REQUIRE(dact_ && y_ && gamma && beta && stats && dgb_partials, TECM_E_ARG, "tecm_groupnorm_gelu_bwd: null pointer");
  const GnPlan p = gn_bwd_plan(B, L, N, Cout, dstride, io_bf16, seq_sums != nullptr, dact_, y_, dy_);
  TECM_REQUIRE(p.kernel != GN_NONE, TECM_E_ARG, "tecm_groupnorm_gelu_bwd: %s (got L = %d, Cout = %d)", p.why, L, Cout);
  const int L2 = (L + dstride - 1) / dstride;
  hipStream_t st = (hipStream_t)stream;
  with_cpb(p.cpb, [&](auto cpb) {
    constexpr int CPB = decltype(cpb)::value;
    // every kernel that writes dy in one launch: nb blocks (the register kernels also take the pairs per lane)
    auto go = [&](auto kern, auto... tail) {
      hipLaunchKernelGGL(kern, dim3(nb), dim3(p.nthr), 0, st, dact_, dstride, L2, y_, gamma, beta, stats, dy_, dgb_partials, B, L, N,
                         tail...);
    };
    auto reg = [&](auto wps) {
      constexpr int WPS = decltype(wps)::value;
      if (p.y16) go(gn_gelu_bwd_reg<CPB, WPS, 9, true, true, true>, p.np);
      else if (p.d16) go(gn_gelu_bwd_reg<CPB, WPS, 9, true, true>, p.np);
      else if (p.io16) go(gn_gelu_bwd_reg<CPB, WPS, 9, true>, p.np);
      else go(gn_gelu_bwd_reg<CPB, WPS, 9, false>, p.np);
    };
    if (p.kernel == GN_SPLIT16) {
      if constexpr (CPB <= 2) {                          // (the plan asks for Cout 64 or 128)
        // items = (sample, node group)
        const int npb = CPB == 1 ? 10 : 5;
        const int items = B * ((N + npb - 1) / npb);
        const int active = items < nb ? items : nb;     // (an even deal -- 779 blocks of 3 items instead of 1024 of 2-3 --
                                                        //  measured 145 us against 121: fewer waves in flight cost more)
        hipLaunchKernelGGL(gn_bwd_sums16_kernel<CPB>, dim3(nb), dim3(256), 0, st, dact_, dstride, L2, y_, gamma, beta, stats, seq_sums,
                           dgb_partials, B, L, N, active);
        hipLaunchKernelGGL(gn_bwd_apply16_kernel<CPB>, dim3(nb), dim3(256), 0, st, dact_, dstride, L2, y_, gamma, beta, stats, seq_sums,
                           dy_, dgb_partials, B, L, N);
      }
    } else if (p.kernel == GN_REG) {
      if (p.wps == 4) reg(std::integral_constant<int, 4>{}); else reg(std::integral_constant<int, 8>{});
    } else if (p.kernel == GN_REG16) {
      if (p.ng == 3) go(gn_gelu_bwd_reg16<CPB, 3>); else go(gn_gelu_bwd_reg16<CPB, 6>);
    } else {
      hipLaunchKernelGGL(gn_gelu_bwd_kernel<CPB>, dim3(nb), dim3(256), 0, st, reinterpret_cast<const float*>(dact_), dstride, L2,
                         reinterpret_cast<const float*>(y_), gamma, beta, stats, reinterpret_cast<float*>(dy_), dgb_partials, B, L, N);
    }
  });
  TECM_CHECK_LAUNCH(gn_plan_name(p, "bwd"));
  return TECM_OK;
}
