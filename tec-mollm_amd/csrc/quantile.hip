// Quantile forecasts (include/tecmollm.h (3k)): the kernels under PinballFn / PinballLoss (tecmollm/functions.py),
// QuantileMetrics (src/evaluation/metrics.py) and calibrate_cqr (tecmollm/quantile.py).
//
//   pinball_stage1_kernel / pinball_stage2_kernel  (a)  mean pinball loss + gradient of the head's permuted (B, Q, H, N) view.
//       Block (x, q): the level is block-uniform, so tau_q is one scalar and a level's sum is a run of the workspace; the
//       elements of a level are walked in pred's storage order (h fastest for the head's (B, N, Q*H) storage).  float64
//       partials: wave butterfly, (w0 + w1) + (w2 + w3), one double per block; stage 2 is one block over the Q * nbx partials.
//   quantile_stats_kernel<QP>                      (b)  the shape of ensemble_stats_kernel: block = one wave = (tile of 64
//       nodes, horizon, group), a thread owns cell (g, h, i), walks the samples in ascending s and adds once at the end.
//   quantile_scores_kernel<QP>                     (c)  elementwise, block = 64 nodes x 4 horizons, blockIdx.z strides over
//       the samples: the addressing of conformal_scores_kernel.
//
// (b) and (c) take the levels through ONE device function, quantile_sorted<QP>: value pipeline, crossing flag, sort, adjust.
// The Q levels of a cell live in a register array of the compile-time size QP = 1, 2, 4, 8 or 16 >= Q, padded with +inf
// (the pipeline leaves finite values, so the padding sorts last), and go through the unrolled bitonic network of
// ensemble.hip.  z_{Q-1-r}, a run-time position, is picked by an unrolled compare-and-select, never by an indexed read: no
// instance uses scratch (a ceiling of __graft_entry__.py).
#include <limits>

#include "common.h"
#include "metrics_value.h"

namespace {

// ------------------------------------------------------------------------------------------------ (a)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void pinball_stage1_kernel(TecmPinball p, int64_t M, float g) {
  __shared__ double red[4];
  const int q = blockIdx.y;
  const float tau = p.taus[q];
  const double taud = (double)tau;
  const bool n_fast = p.p_stride_n == 1;
  const int64_t inner = n_fast ? p.N : p.H, plane = (int64_t)p.H * p.N;
  const float* pred = p.pred + (int64_t)q * p.p_stride_q;
  float* dpred = p.dpred ? p.dpred + (int64_t)q * p.p_stride_q : nullptr;
  double acc = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < M; e += (int64_t)gridDim.x * 256) {
    const int64_t b = e / plane, rem = e - b * plane;
    const int64_t outer = rem / inner, in = rem - outer * inner;
    const int64_t h = n_fast ? outer : in, n = n_fast ? in : outer;
    const int64_t ip = b * p.p_stride_b + h * p.p_stride_h + n * p.p_stride_n;
    const float u = p.target[b * p.t_stride_b + h * p.t_stride_h + n * p.t_stride_n] - pred[ip];
    const bool neg = u < 0.f;
    acc += (double)u * (taud - (neg ? 1.0 : 0.0));
    if (dpred) dpred[ip] = g * ((neg ? 1.f : 0.f) - tau);
  }
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) p.workspace[(int64_t)q * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void pinball_stage2_kernel(TecmPinball p, int nbx, double M) {
  __shared__ double red[4];
  double total = 0.0;                        // thread 0 only
  for (int q = 0; q < p.Q; ++q) {
    double acc = 0.0;
    for (int x = threadIdx.x; x < nbx; x += 256) acc += p.workspace[(int64_t)q * nbx + x];
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      const double level = (red[0] + red[1]) + (red[2] + red[3]);
      if (p.loss_levels) p.loss_levels[q] = (float)(level / M);
      total += level;
    }
    __syncthreads();                         // red is read before the next level overwrites it
  }
  if (threadIdx.x == 0) p.loss_out[0] = (float)(total / ((double)p.Q * M));
}

// ------------------------------------------------------------------------------------------------ (b), (c)
constexpr int QT_TILE = 64;                  // nodes per block of (b) and per wave of (c) = lanes of a wave
constexpr int QT_HC = 4;                     // horizons per block of (c) = waves

template <int KP>
__device__ __forceinline__ void sort_network(float (&v)[KP]) {
#pragma unroll
  for (int size = 2; size <= KP; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        const int p = j ^ stride;
        if (p > j) {
          const float lo = fminf(v[j], v[p]), hi = fmaxf(v[j], v[p]);
          const bool up = (j & size) == 0;   // ascending half of this merge
          v[j] = up ? lo : hi;
          v[p] = up ? hi : lo;
        }
      }
    }
  }
}

// raw scaled levels x[0..Q) (entries at and beyond Q are ignored) and raw target -> the sorted (and adjusted) levels z in
// physical units, +inf beyond Q, the target y, and whether the levels crossed.  adjust points at the cell's first level,
// adj_stride apart, or is NULL.
template <int QP>
__device__ __forceinline__ void quantile_sorted(const float (&x)[QP], float yraw, int Q, double mean, double scale, int clip,
                                                float clip_lo, float clip_hi, const float* adjust, int64_t adj_stride,
                                                float (&z)[QP], float& y, bool& crossing) {
  const float INF = std::numeric_limits<float>::infinity();
#pragma unroll
  for (int q = 0; q < QP; ++q) {
    z[q] = INF;
    if (q < Q) {
      float v = x[q];
      if (!isfinite(v)) v = 0.f;
      v = nan_to_num_tec(unscale_f32(v, mean, scale));
      if (clip) v = fminf(fmaxf(v, clip_lo), clip_hi);
      z[q] = v;
    }
  }
  y = nan_to_num_tec(unscale_f32(yraw, mean, scale));
  crossing = false;
#pragma unroll
  for (int q = 0; q + 1 < QP; ++q)
    if (q + 1 < Q && z[q] > z[q + 1]) crossing = true;
  sort_network<QP>(z);
  if (adjust) {
#pragma unroll
    for (int q = 0; q < QP; ++q)
      if (q < Q) z[q] = z[q] + adjust[(int64_t)q * adj_stride];
  }
}

// z[idx] for a run-time idx without an indexed register read
template <int QP>
__device__ __forceinline__ float pick(const float (&z)[QP], int idx) {
  float v = z[0];
#pragma unroll
  for (int j = 1; j < QP; ++j) v = j == idx ? z[j] : v;
  return v;
}

template <int QP>
__global__ __launch_bounds__(QT_TILE) void quantile_stats_kernel(TecmQuantileStats c) {
  constexpr int PP = QP / 2 > 0 ? QP / 2 : 1;
  const unsigned lane = threadIdx.x;
  const int g = blockIdx.z;
  const int64_t h = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * QT_TILE + lane;
  const bool own = i < c.I;                  // this thread's cell is (g, h, i)
  const int Q = c.Q, P = Q / 2;
  const bool score = c.target != nullptr;

  double cnt = 0.0, rho[QP], wid[PP];
  uint32_t ncross = 0u, hits[QP], cov[PP];
#pragma unroll
  for (int q = 0; q < QP; ++q) {
    rho[q] = 0.0;
    hits[q] = 0u;
  }
#pragma unroll
  for (int r = 0; r < PP; ++r) {
    wid[r] = 0.0;
    cov[r] = 0u;
  }
  const float* adjust = nullptr;
  if (c.adjust && own) adjust = c.adjust + (((int64_t)(c.Ga == c.G ? g : 0) * c.H + h) * Q) * c.I + i;

  bool present = false, bad = false;
  for (int64_t s = 0; s < c.S; ++s) {
    const int id = c.group ? c.group[s] : 0;     // block-uniform
    if ((unsigned)id >= (unsigned)c.G) bad = true;
    if (id != g) continue;
    present = true;
    if (!own) continue;
    float x[QP];
    const float* base = c.levels + s * c.l_stride_s + h * c.l_stride_h + i * c.l_stride_i;
#pragma unroll
    for (int q = 0; q < QP; ++q) x[q] = q < Q ? base[(int64_t)q * c.l_stride_q] : 0.f;
    const float yraw = score ? c.target[s * c.t_stride_s + h * c.t_stride_h + i * c.t_stride_i] : 0.f;
    float z[QP], y;
    bool crossing;
    quantile_sorted<QP>(x, yraw, Q, c.mean, c.scale, c.clip, c.clip_lo, c.clip_hi, adjust, c.I, z, y, crossing);
    if (c.out_z) {
      float* o = c.out_z + s * c.o_stride_s + h * c.o_stride_h + i * c.o_stride_i;
#pragma unroll
      for (int q = 0; q < QP; ++q)
        if (q < Q) o[(int64_t)q * c.o_stride_q] = z[q];
    }
    if (!score) continue;
    cnt += 1.0;
    ncross += crossing ? 1u : 0u;
    const double yd = y;
#pragma unroll
    for (int q = 0; q < QP; ++q) {
      if (q < Q) {
        rho[q] += (yd - (double)z[q]) * ((double)c.taus[q] - (y < z[q] ? 1.0 : 0.0));
        hits[q] += y <= z[q] ? 1u : 0u;
      }
    }
#pragma unroll
    for (int r = 0; r < PP; ++r) {
      if (r < P) {
        const float lo = z[r], hi = pick<QP>(z, Q - 1 - r);
        wid[r] += (double)hi - (double)lo;
        cov[r] += (lo <= y && y <= hi) ? 1u : 0u;
      }
    }
  }
  if (bad && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) atomicOr(c.err_flag, TECM_BAD_GROUP);
  if (!present || !own || !score) return;
  const int64_t rows = 1 + Q + P, cell0 = (((int64_t)g * c.H + h) * rows) * c.I + i;
  double* st = c.stats + cell0;
  uint32_t* ct = c.counts + cell0;
  st[0] += cnt;
  ct[0] += ncross;
#pragma unroll
  for (int q = 0; q < QP; ++q) {
    if (q < Q) {
      st[(int64_t)(1 + q) * c.I] += rho[q];
      ct[(int64_t)(1 + q) * c.I] += hits[q];
    }
  }
#pragma unroll
  for (int r = 0; r < PP; ++r) {
    if (r < P) {
      st[(int64_t)(1 + Q + r) * c.I] += wid[r];
      ct[(int64_t)(1 + Q + r) * c.I] += cov[r];
    }
  }
}

template <int QP>
__global__ __launch_bounds__(256) void quantile_scores_kernel(TecmQuantileScores c) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * QT_TILE + lane, h = (int64_t)blockIdx.y * QT_HC + wave;
  if (i >= c.I || h >= c.H) return;
  const int Q = c.Q;
  for (int64_t s = blockIdx.z; s < c.S; s += gridDim.z) {
    float x[QP];
    const float* base = c.levels + s * c.l_stride_s + h * c.l_stride_h + i * c.l_stride_i;
#pragma unroll
    for (int q = 0; q < QP; ++q) x[q] = q < Q ? base[(int64_t)q * c.l_stride_q] : 0.f;
    const float yraw = c.target[s * c.t_stride_s + h * c.t_stride_h + i * c.t_stride_i];
    float z[QP], y;
    bool crossing;
    quantile_sorted<QP>(x, yraw, Q, c.mean, c.scale, c.clip, c.clip_lo, c.clip_hi, nullptr, 0, z, y, crossing);
    const float lo = pick<QP>(z, c.lo_idx), hi = pick<QP>(z, c.hi_idx);
    c.scores[(c.row0 + s) * c.ld + h * c.I + i] = fmaxf(lo - y, y - hi);
  }
}

template <int QP>
void launch_stats(const TecmQuantileStats* c, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL(quantile_stats_kernel<QP>, grid, dim3(QT_TILE), 0, stream, *c);
}
template <int QP>
void launch_scores(const TecmQuantileScores* c, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL(quantile_scores_kernel<QP>, grid, dim3(256), 0, stream, *c);
}

bool taus_ok(const float* taus, int Q) {
  for (int q = 0; q < Q; ++q) {
    if (!(taus[q] > 0.f && taus[q] < 1.f)) return false;
    if (q > 0 && !(taus[q - 1] < taus[q])) return false;
  }
  return true;
}

}  // namespace

extern "C" int tecm_pinball_fwd_bwd_strided(const TecmPinball* p, void* stream) {
  TECM_REQUIRE(p, TECM_E_ARG, "tecm_pinball_fwd_bwd_strided: null descriptor");
  TECM_REQUIRE(p->pred && p->target && p->loss_out && p->workspace, TECM_E_ARG, "tecm_pinball_fwd_bwd_strided: null pointer");
  TECM_REQUIRE(p->B > 0 && p->H > 0 && p->N > 0, TECM_E_ARG, "tecm_pinball_fwd_bwd_strided: bad shape");
  TECM_REQUIRE(p->Q >= 1 && p->Q <= TECM_QUANT_MAX_Q, TECM_E_ARG, "tecm_pinball_fwd_bwd_strided: Q = %d outside [1, %d]",
               (int)p->Q, TECM_QUANT_MAX_Q);
  TECM_REQUIRE(taus_ok(p->taus, p->Q), TECM_E_ARG,
               "tecm_pinball_fwd_bwd_strided: the levels must increase strictly inside (0, 1)");
  const int64_t M = (int64_t)p->B * p->H * p->N;
  TECM_REQUIRE(M <= ((int64_t)1 << 53) / p->Q, TECM_E_ARG, "tecm_pinball_fwd_bwd_strided: Q * B * H * N must stay below 2^53");
  TECM_REQUIRE(tecm_aligned(p->pred, 4) && tecm_aligned(p->target, 4) && tecm_aligned(p->dpred, 4) &&
                   tecm_aligned(p->loss_out, 4) && tecm_aligned(p->loss_levels, 4) && tecm_aligned(p->workspace, 8),
               TECM_E_ALIGN, "tecm_pinball_fwd_bwd_strided: float operands must be 4-byte, the workspace 8-byte aligned");
  const int64_t want = (M + 255) / 256;
  const int nbx = (int)(want < TECM_PINBALL_BLOCK_CAP ? want : TECM_PINBALL_BLOCK_CAP);
  hipStream_t st = (hipStream_t)stream;
  const float g = p->grad_scale / (float)(M * p->Q);
  hipLaunchKernelGGL(pinball_stage1_kernel, dim3((unsigned)nbx, (unsigned)p->Q), dim3(256), 0, st, *p, M, g);
  TECM_CHECK_LAUNCH("tecm_pinball_fwd_bwd_strided/stage1");
  hipLaunchKernelGGL(pinball_stage2_kernel, dim3(1), dim3(256), 0, st, *p, nbx, (double)M);
  TECM_CHECK_LAUNCH("tecm_pinball_fwd_bwd_strided/stage2");
  return TECM_OK;
}

extern "C" int tecm_quantile_stats(const TecmQuantileStats* c, void* stream) {
  TECM_REQUIRE(c, TECM_E_ARG, "tecm_quantile_stats: null descriptor");
  TECM_REQUIRE(c->levels && c->err_flag, TECM_E_ARG, "tecm_quantile_stats: null pointer");
  TECM_REQUIRE(c->target ? (c->stats && c->counts) : c->out_z != nullptr, TECM_E_ARG,
               "tecm_quantile_stats: a target needs stats and counts, no target needs out_z");
  TECM_REQUIRE(c->S > 0 && c->H > 0 && c->I > 0 && c->G > 0, TECM_E_ARG, "tecm_quantile_stats: bad shape");
  TECM_REQUIRE(c->Q >= 1 && c->Q <= TECM_QUANT_MAX_Q, TECM_E_ARG, "tecm_quantile_stats: Q = %d outside [1, %d]", (int)c->Q,
               TECM_QUANT_MAX_Q);
  TECM_REQUIRE(taus_ok(c->taus, c->Q), TECM_E_ARG, "tecm_quantile_stats: the levels must increase strictly inside (0, 1)");
  TECM_REQUIRE(!c->adjust || c->Ga == 1 || c->Ga == c->G, TECM_E_ARG, "tecm_quantile_stats: Ga must be 1 or G");
  const int64_t tiles = (c->I + QT_TILE - 1) / QT_TILE;
  TECM_REQUIRE(c->G <= 65535 && c->H <= 65535, TECM_E_ARG, "tecm_quantile_stats: G and H must be <= 65535");
  TECM_REQUIRE(tiles < (1 << 24) && tiles * c->H < (1 << 24) && tiles * c->H * c->G < (1 << 24), TECM_E_ARG,
               "tecm_quantile_stats: more than 2^24 blocks of 64 threads");
  TECM_REQUIRE(c->I <= INT64_MAX / (int64_t)sizeof(double) / (2 * TECM_QUANT_MAX_Q) / c->H / c->G, TECM_E_ARG,
               "tecm_quantile_stats: G * H * (1 + Q + Q / 2) * I doubles do not fit 64-bit addressing");
  TECM_REQUIRE(c->scale != 0.0, TECM_E_ARG, "tecm_quantile_stats: scale must be non-zero");
  TECM_REQUIRE(tecm_aligned(c->stats, 8) && tecm_aligned(c->counts, 4) && tecm_aligned(c->group, 4) &&
                   tecm_aligned(c->err_flag, 4),
               TECM_E_ALIGN, "tecm_quantile_stats: stats must be 8-byte aligned, counts, group and err_flag 4-byte aligned");
  TECM_REQUIRE(tecm_aligned(c->levels, 4) && tecm_aligned(c->target, 4) && tecm_aligned(c->adjust, 4) && tecm_aligned(c->out_z, 4),
               TECM_E_ALIGN, "tecm_quantile_stats: levels, target, adjust and out_z must be 4-byte aligned");
  const dim3 grid((unsigned)tiles, (unsigned)c->H, (unsigned)c->G);
  hipStream_t st = (hipStream_t)stream;
  if (c->Q <= 1) launch_stats<1>(c, grid, st);
  else if (c->Q <= 2) launch_stats<2>(c, grid, st);
  else if (c->Q <= 4) launch_stats<4>(c, grid, st);
  else if (c->Q <= 8) launch_stats<8>(c, grid, st);
  else launch_stats<16>(c, grid, st);
  TECM_CHECK_LAUNCH("tecm_quantile_stats");
  return TECM_OK;
}

extern "C" int tecm_quantile_scores(const TecmQuantileScores* c, void* stream) {
  TECM_REQUIRE(c, TECM_E_ARG, "tecm_quantile_scores: null descriptor");
  TECM_REQUIRE(c->levels && c->target && c->scores, TECM_E_ARG, "tecm_quantile_scores: null pointer");
  TECM_REQUIRE(c->S > 0 && c->H > 0 && c->I > 0, TECM_E_ARG, "tecm_quantile_scores: bad shape");
  TECM_REQUIRE(c->Q >= 1 && c->Q <= TECM_QUANT_MAX_Q, TECM_E_ARG, "tecm_quantile_scores: Q = %d outside [1, %d]", (int)c->Q,
               TECM_QUANT_MAX_Q);
  TECM_REQUIRE(c->lo_idx >= 0 && c->lo_idx <= c->hi_idx && c->hi_idx < c->Q, TECM_E_ARG,
               "tecm_quantile_scores: needs 0 <= lo_idx <= hi_idx < Q");
  TECM_REQUIRE(c->I <= INT64_MAX / (int64_t)sizeof(float) / c->H && c->ld >= (int64_t)c->H * c->I && c->row0 >= 0 &&
                   c->row0 + c->S <= INT64_MAX / (int64_t)sizeof(float) / c->ld,
               TECM_E_ARG, "tecm_quantile_scores: needs ld >= H * I, row0 >= 0 and a store within 64-bit addressing");
  TECM_REQUIRE(c->scale != 0.0, TECM_E_ARG, "tecm_quantile_scores: scale must be non-zero");
  TECM_REQUIRE(tecm_aligned(c->levels, 4) && tecm_aligned(c->target, 4) && tecm_aligned(c->scores, 4), TECM_E_ALIGN,
               "tecm_quantile_scores: levels, target and scores must be 4-byte aligned");
  const int64_t chunks = ((int64_t)c->H + QT_HC - 1) / QT_HC, tiles = (c->I + QT_TILE - 1) / QT_TILE;
  TECM_REQUIRE(chunks <= 65535 && tiles < (1 << 24), TECM_E_ARG,
               "tecm_quantile_scores: ceil(H / 4) must be <= 65535 and ceil(I / 64) < 2^24");
  const dim3 grid((unsigned)tiles, (unsigned)chunks, (unsigned)(c->S < 1024 ? c->S : 1024));
  hipStream_t st = (hipStream_t)stream;
  if (c->Q <= 1) launch_scores<1>(c, grid, st);
  else if (c->Q <= 2) launch_scores<2>(c, grid, st);
  else if (c->Q <= 4) launch_scores<4>(c, grid, st);
  else if (c->Q <= 8) launch_scores<8>(c, grid, st);
  else launch_scores<16>(c, grid, st);
  TECM_CHECK_LAUNCH("tecm_quantile_scores");
  return TECM_OK;
}
