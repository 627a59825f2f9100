// Probabilistic scores of a K-member ensemble per cell (group, horizon, node): tecm_ensemble_stats (include/tecmollm.h
// (3c)), the kernel under EnsembleMetrics (src/evaluation/metrics.py) -- CRPS, spread, interval coverage and the rank
// histogram without a host copy of the members.  A streaming kernel: K + 1 floats read per (sample, horizon, node).
//
// Block (x, y, z) = (tile of 64 nodes, horizon h, group g), ONE wave: lane = node of the tile, so a thread owns one cell
// (g, h, i) and keeps its nine sums in registers and its K + 1 rank counters in a column of LDS that only it touches
// (the rank is a run-time index; at most 16.25 KiB per block).  The waves share nothing, so one
// wave per block spreads N = 2911, H = 12 over 552 blocks instead of 138.  A thread walks the samples in ascending s,
// takes those whose group is g, and adds its sums to `stats` / `hist` once at the end: one owner per cell, no atomics, a
// fixed order.  A block whose group does not occur among the S ids touches no statistics.  While the members of one
// sample are sorted, the K + 1 loads of the block's next sample are already in flight (cur / nxt below; up to K = 16).
//
// The K members of a cell live in a register array of the compile-time size KP = 2, 4, 8, 16, 32 or 64 >= K, padded with
// +inf (every value the pipeline of metrics_value.h leaves is finite, so the padding sorts behind the members), and go
// through a fully unrolled bitonic network: every index is a compile-time constant, no instance uses scratch (a ceiling
// of __graft_entry__.py).  Rank and mean_raw are taken before the sort; every sum over members runs over the sorted array
// in ascending order, in float64.
//
// Lanes run along the nodes: members with stride_i == 1 (what ensemble_members returns) are read as 64 consecutive floats
// per wave and member.  Every other stride combination of either operand -- the model's permuted view (stride_h == 1,
// stride_i == H) among them -- is read in place with the coalescing its strides give: the target is one of K + 1 operands
// and the H neighbouring blocks of a tile read the same lines of it, so it is not staged.
//
// Measured at N = 2911, H = 12, B = 16, one group (profiles/ensemble.txt): 47 / 80 / 186 us for K = 8 / 16 / 32, 0.47-0.60 TB/s
// of algorithmic bytes -- a tenth of what HBM delivers.  The kernel is bound by each wave's serial walk over its 16 samples
// (a load round trip, the float64 sums and three divisions per sample; one or two waves per SIMD), not by bytes: the order
// of the samples within a cell is fixed by contract, so the way on is more samples in flight per wave, not more waves per
// cell.  One update is below 0.1 % of the K forwards it follows, and its launch costs more than its run.
#include <limits>

#include "common.h"
#include "metrics_value.h"

namespace {

constexpr int ENS_TILE = 64;                 // nodes per block = lanes of the wave

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

template <int KP>
__global__ __launch_bounds__(ENS_TILE) void ensemble_stats_kernel(TecmEnsemble q) {
  const unsigned lane = threadIdx.x;
  const int g = blockIdx.z;
  const int64_t h = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * ENS_TILE + lane;
  const bool own = i < q.I;                  // this thread's cell is (g, h, i)
  const int K = q.K, m = q.trim;
  const double dK = (double)K;
  const float INF = std::numeric_limits<float>::infinity();

  double a[TECM_ENS_STATS];
#pragma unroll
  for (int n = 0; n < TECM_ENS_STATS; ++n) a[n] = 0.0;
  __shared__ uint32_t cnt[(KP + 1) * ENS_TILE];   // [rank][lane]: a thread touches its own column only, no barrier
#pragma unroll
  for (int r = 0; r <= KP; ++r) cnt[r * ENS_TILE + lane] = 0u;

  bool bad = false;
  // the block's next sample at or after s (block-uniform); every id is looked at exactly once
  auto next_match = [&](int64_t s) {
    for (; s < q.S; ++s) {
      const int id = q.group ? q.group[s] : 0;
      if ((unsigned)id >= (unsigned)q.G) bad = true;
      if (id == g) break;
    }
    return s;
  };
  auto load = [&](auto& x, float& y, int64_t s) {
    // block-uniform base + the lane's offset: with contiguous nodes the offset is the lane itself, one register for all K
    const float* base = q.members + s * q.m_stride_s + h * q.m_stride_h + (int64_t)blockIdx.x * ENS_TILE * q.m_stride_i;
    if (q.m_stride_i == 1) {
#pragma unroll
      for (int k = 0; k < KP; ++k) x[k] = (own && k < K) ? (base + (int64_t)k * q.m_stride_k)[lane] : INF;
    } else {
      const int64_t off = (int64_t)lane * q.m_stride_i;
#pragma unroll
      for (int k = 0; k < KP; ++k) x[k] = (own && k < K) ? (base + (int64_t)k * q.m_stride_k)[off] : INF;
    }
    y = own ? q.target[s * q.t_stride_s + h * q.t_stride_h + i * q.t_stride_i] : 0.f;
  };

  constexpr bool PREFETCH = KP <= 16;        // two samples of 32 or 64 members do not fit the register file next to the sort
  constexpr int KN = PREFETCH ? KP : 1;
  float cur[KP], nxt[KN], ycur = 0.f, ynxt = 0.f;
#pragma unroll
  for (int k = 0; k < KP; ++k) cur[k] = INF;
#pragma unroll
  for (int k = 0; k < KN; ++k) nxt[k] = INF;
  int64_t s = next_match(0);
  const bool present = s < q.S;
  if constexpr (PREFETCH)
    if (present) load(cur, ycur, s);
  while (s < q.S) {
    const int64_t s2 = next_match(s + 1);
    if constexpr (PREFETCH) {
      if (s2 < q.S) load(nxt, ynxt, s2);
    } else {
      load(cur, ycur, s);
    }
    if (own) {
      // value pipeline (metrics_value.h), member order
      float v[KP];
      double raw = 0.0;
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        v[k] = INF;
        if (k < K) {
          float p32 = cur[k];
          if (!isfinite(p32)) p32 = 0.f;
          raw += (double)p32;
          p32 = nan_to_num_tec(unscale_f32(p32, q.mean, q.scale));
          if (q.clip) p32 = fminf(fmaxf(p32, q.clip_lo), q.clip_hi);
          v[k] = p32;
        }
      }
      const float y32 = nan_to_num_tec(unscale_f32(ycur, q.mean, q.scale));
      const double y = y32;
      int lt = 0, eq = 0;                    // the padding is +inf and y32 is finite: it counts in neither
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        lt += v[k] < y32;
        eq += v[k] == y32;
      }
      const int rank = lt + (eq >> 1);       // mid-rank, in [0, K]
      cnt[rank * ENS_TILE + lane] += 1u;
      sort_network<KP>(v);
      double sum = 0.0;
#pragma unroll
      for (int j = 0; j < KP; ++j)
        if (j < K) sum += (double)v[j];
      const double mu = sum / dK;
      // (the second pass converts the members again: kept as doubles across the division they would take 2 KP registers)
#pragma unroll
      for (int j = 0; j < KP; ++j) asm volatile("" : "+v"(v[j]));
      double ss = 0.0, sa = 0.0, D = 0.0;
      float lo = 0.f, hi = 0.f;
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        if (j < K) {
          const double x = v[j], d = x - mu;
          ss += d * d;
          sa += fabs(x - y);
          D += (double)(2 * (j + 1) - K - 1) * x;
        }
        if (j == m) lo = v[j];
        if (j == K - 1 - m) hi = v[j];
      }
      const double var = ss / (dK - 1.0), A = sa / dK, e = mu - y, width = (double)hi - (double)lo;
      a[0] += 1.0; a[1] += y; a[2] += mu; a[3] += e * e; a[4] += fabs(e); a[5] += var; a[6] += A; a[7] += D; a[8] += width;
      const int64_t o = s * q.o_stride_s + h * q.o_stride_h + i * q.o_stride_i;
      if (q.out_mean) q.out_mean[o] = (float)mu;
      if (q.out_std) q.out_std[o] = (float)sqrt(var);
      if (q.out_lo) q.out_lo[o] = lo;
      if (q.out_hi) q.out_hi[o] = hi;
      if (q.out_mean_raw) q.out_mean_raw[o] = (float)(raw / dK);
    }
    if constexpr (PREFETCH) {
#pragma unroll
      for (int k = 0; k < KP; ++k) cur[k] = nxt[k];
      ycur = ynxt;
    }
    s = s2;
  }
  if (bad && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) atomicOr(q.err_flag, TECM_BAD_GROUP);
  if (!present || !own) return;
  double* cell = q.stats + (((int64_t)g * q.H + h) * TECM_ENS_STATS) * q.I + i;
#pragma unroll
  for (int n = 0; n < TECM_ENS_STATS; ++n) cell[(int64_t)n * q.I] += a[n];
  uint32_t* bins = q.hist + (((int64_t)g * q.H + h) * (K + 1)) * q.I + i;
  for (int r = 0; r <= K; ++r) bins[(int64_t)r * q.I] += cnt[r * ENS_TILE + lane];
}

template <int KP>
void launch(const TecmEnsemble* e, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL(ensemble_stats_kernel<KP>, grid, dim3(ENS_TILE), 0, stream, *e);
}

}  // namespace

extern "C" int tecm_ensemble_stats(const TecmEnsemble* e, void* stream) {
  TECM_REQUIRE(e, TECM_E_ARG, "tecm_ensemble_stats: null descriptor");
  TECM_REQUIRE(e->members && e->target && e->stats && e->hist && e->err_flag, TECM_E_ARG,
               "tecm_ensemble_stats: null pointer");
  TECM_REQUIRE(e->S > 0 && e->H > 0 && e->I > 0 && e->G > 0, TECM_E_ARG, "tecm_ensemble_stats: bad shape");
  TECM_REQUIRE(e->K >= 2 && e->K <= TECM_ENS_MAX_K, TECM_E_ARG, "tecm_ensemble_stats: K = %d outside [2, %d]", (int)e->K,
               TECM_ENS_MAX_K);
  TECM_REQUIRE(e->trim >= 0 && 2 * (int64_t)e->trim < (int64_t)e->K - 1, TECM_E_ARG,
               "tecm_ensemble_stats: trim = %d, needs 0 <= 2 * trim < K - 1 = %d", (int)e->trim, (int)e->K - 1);
  const int64_t tiles = (e->I + ENS_TILE - 1) / ENS_TILE;
  TECM_REQUIRE(e->G <= 65535 && e->H <= 65535, TECM_E_ARG, "tecm_ensemble_stats: G and H must be <= 65535");
  TECM_REQUIRE(tiles < (1 << 24) && tiles * e->H < (1 << 24) && tiles * e->H * e->G < (1 << 24), TECM_E_ARG,
               "tecm_ensemble_stats: more than 2^24 blocks of 64 threads");
  TECM_REQUIRE(e->I <= INT64_MAX / (int64_t)sizeof(double) / (TECM_ENS_MAX_K + 1) / e->H / e->G, TECM_E_ARG,
               "tecm_ensemble_stats: G * H * 9 * I doubles or G * H * (K + 1) * I counts do not fit 64-bit addressing");
  TECM_REQUIRE(e->scale != 0.0, TECM_E_ARG, "tecm_ensemble_stats: scale must be non-zero");
  TECM_REQUIRE(tecm_aligned(e->stats, 8) && tecm_aligned(e->hist, 4) && tecm_aligned(e->group, 4) &&
                   tecm_aligned(e->err_flag, 4),
               TECM_E_ALIGN, "tecm_ensemble_stats: stats must be 8-byte aligned, hist, group and err_flag 4-byte aligned");
  TECM_REQUIRE(tecm_aligned(e->members, 4) && tecm_aligned(e->target, 4) && tecm_aligned(e->out_mean, 4) &&
                   tecm_aligned(e->out_std, 4) && tecm_aligned(e->out_lo, 4) && tecm_aligned(e->out_hi, 4) &&
                   tecm_aligned(e->out_mean_raw, 4),
               TECM_E_ALIGN, "tecm_ensemble_stats: members, target and the per-sample outputs must be 4-byte aligned");
  const dim3 grid((unsigned)tiles, (unsigned)e->H, (unsigned)e->G);
  hipStream_t st = (hipStream_t)stream;
  if (e->K <= 2) launch<2>(e, grid, st);
  else if (e->K <= 4) launch<4>(e, grid, st);
  else if (e->K <= 8) launch<8>(e, grid, st);
  else if (e->K <= 16) launch<16>(e, grid, st);
  else if (e->K <= 32) launch<32>(e, grid, st);
  else launch<64>(e, grid, st);
  TECM_CHECK_LAUNCH("tecm_ensemble_stats");
  return TECM_OK;
}
