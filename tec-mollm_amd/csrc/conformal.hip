// Split-conformal prediction intervals (include/tecmollm.h (3g)): the kernels under tecmollm/conformal.py and
// IntervalMetrics (src/evaluation/metrics.py).
//
//   conformal_scores_kernel  (a)  scores of one batch into rows of the score store; elementwise, block = 64 nodes x 4 horizons,
//                                 blockIdx.z strides over the samples; operands read in place through their strides.
//   column_select_kernel     (b)  the exact k-th smallest per (group, column) of the store: the hot path, see below.
//   interval_stats_kernel    (c)  the shape of metrics_map_kernel: block = (64 nodes, 4 horizons, group), one owner per cell
//                                 walking the samples in ascending s, eight in flight, one add to `stats` at the end.
//
// column_select_kernel: a four-pass most-significant-digit radix select on 8-bit digits of the monotone key.  Block (x, y, z)
// = (tile of 64 columns, group g, rank q), 16 waves: lane = column, so a row of the tile is one coalesced 256-B read.  The
// waves take the rows in chunks of eight (wave w: rows 128 n + 8 w .. + 7), test the eight group ids -- wave-uniform, read on
// the scalar path, so rows of other groups are never loaded --, issue the up to eight row loads together and then count the
// digit of every element whose higher digits equal the prefix found so far into hist[digit][lane] with LDS integer adds: the
// 64 lanes of a wave hit 64 different banks.  After the pass wave w sums segment w (16 bins) of its lane's column into
// part[w][lane]; then EVERY wave finds, for its lane's column, the segment that holds the rank from the 16 partial sums and
// walks that segment's 16 bins: all waves end the pass with the column's new prefix and reduced rank in registers and
// nothing is broadcast.  The total of pass 0 is the number of rows of the group, which settles rank > n.  Counts are
// integers, so the result does not depend on the order in which the waves add.  LDS: 64 KiB + 4 KiB per block, two blocks
// and so 32 waves per CU.
// (Four waves per block, the first cut, took 889 us for the 300 MB store of the full split -- 546 tiles are 1.07 rounds of the
// 512 resident blocks, so the last 34 blocks ran a round of their own, and a CU held 8 waves x 8 rows = 16 KiB in flight; 16
// waves per block take 461 us, profiles/conformal.txt: the kernel is bound by the bytes it keeps in flight, not by LDS adds.)
#include <limits>

#include "common.h"
#include "conformal_score.h"

namespace {

constexpr int CF_TILE = 64;                  // nodes per block = lanes of a wave
constexpr int CF_HC = 4;                     // horizons per block = waves
constexpr int CF_SB = 8;                     // samples in flight (c)

__global__ __launch_bounds__(256) void conformal_scores_kernel(TecmConformalScores q) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * CF_TILE + lane, h = (int64_t)blockIdx.y * CF_HC + wave;
  if (i >= q.I || h >= q.H) return;
  for (int64_t s = blockIdx.z; s < q.S; s += gridDim.z) {
    const float praw = q.pred[s * q.p_stride_s + h * q.p_stride_h + i * q.p_stride_i];
    const float yraw = q.target[s * q.t_stride_s + h * q.t_stride_h + i * q.t_stride_i];
    float w = 1.f;
    if (q.sigma) w = conformal_weight(q.sigma[s * q.g_stride_s + h * q.g_stride_h + i * q.g_stride_i], q.sigma_min);
    float p, y;
    conformal_values(praw, yraw, q.mean, q.scale, q.clip, q.clip_lo, q.clip_hi, p, y);
    q.scores[(q.row0 + s) * q.ld + h * q.I + i] = conformal_score(p, y, q.mode, q.sigma != nullptr, w);
  }
}

// ------------------------------------------------------------------------------------------------ (b)
constexpr int SEL_COLS = 64;                 // columns per block = lanes of a wave
constexpr int SEL_BINS = 256;                // 8-bit digits
constexpr int SEL_ROWS = 8;                  // rows a wave has in flight
constexpr int SEL_WAVES = 16;                // waves per block: 2 blocks x 16 waves fill a CU's 32 wave slots
constexpr int SEL_SEG = SEL_BINS / SEL_WAVES;    // bins one wave sums after a pass
constexpr size_t SEL_LDS = (size_t)(SEL_BINS + SEL_WAVES) * SEL_COLS * sizeof(uint32_t);

// numeric order with -0 < +0 adjacent and every NaN last
__device__ __forceinline__ uint32_t sel_key(float v) {
  const uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(SEL_WAVES * 64) void column_select_kernel(TecmColumnSelect q) {
  extern __shared__ uint32_t sel_lds[];
  uint32_t* hist = sel_lds;                            // [SEL_BINS][SEL_COLS]
  uint32_t* part = sel_lds + SEL_BINS * SEL_COLS;      // [SEL_WAVES][SEL_COLS]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int g = blockIdx.y, qi = blockIdx.z;
  const int64_t c = (int64_t)blockIdx.x * SEL_COLS + lane;
  const bool live = c < q.C;
  const int32_t rank_in = q.ranks[(int64_t)g * q.Q + qi];
  const float* col = q.x + (live ? c : 0);

  uint32_t prefix = 0u, rank = rank_in > 0 ? (uint32_t)rank_in : 1u;
  bool over = false, bad = false;
#pragma unroll 1
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int e = threadIdx.x; e < SEL_BINS * SEL_COLS; e += SEL_WAVES * 64) hist[e] = 0u;
    __syncthreads();
    for (int64_t s0 = (int64_t)wave * SEL_ROWS; s0 < q.S; s0 += SEL_WAVES * SEL_ROWS) {
      uint32_t take = 0u;                              // wave-uniform: which of the SEL_ROWS rows belong to g
#pragma unroll
      for (int j = 0; j < SEL_ROWS; ++j) {
        if (s0 + j < q.S) {
          const int id = q.group ? q.group[s0 + j] : 0;
          if (id == g) take |= 1u << j;
          if ((unsigned)id >= (unsigned)q.G) bad = true;
        }
      }
      if (!take || !live) continue;
      float v[SEL_ROWS];
#pragma unroll
      for (int j = 0; j < SEL_ROWS; ++j) v[j] = (take >> j & 1u) ? col[(s0 + j) * q.ld] : 0.f;
#pragma unroll
      for (int j = 0; j < SEL_ROWS; ++j) {
        if (!(take >> j & 1u)) continue;
        const uint32_t k = sel_key(v[j]);
        const uint32_t high = pass == 0 ? 0u : k >> (shift + 8);
        if (high == prefix) atomicAdd(&hist[((k >> shift) & 255u) * SEL_COLS + lane], 1u);
      }
    }
    __syncthreads();
    uint32_t sum = 0u;
#pragma unroll
    for (int b = 0; b < SEL_SEG; ++b) sum += hist[(wave * SEL_SEG + b) * SEL_COLS + lane];
    part[wave * SEL_COLS + lane] = sum;
    __syncthreads();
    // the segment of SEL_SEG bins that holds the rank, then the bin within it
    // (a rank beyond the total -- `over`, or a dead lane -- walks off the end: digit 255, rank 1; its result is not used)
    uint32_t rr = rank, total = 0u;
    int seg = SEL_WAVES - 1;
    bool found = false;
#pragma unroll
    for (int w = 0; w < SEL_WAVES; ++w) {
      const uint32_t n = part[w * SEL_COLS + lane];
      total += n;
      if (!found) {
        if (rr <= n) {
          seg = w;
          found = true;
        } else {
          rr -= n;
        }
      }
    }
    if (pass == 0) over = rank_in > 0 && (uint32_t)rank_in > total;      // the total is the group's row count
    uint32_t digit = 255u;
    found = false;
    const uint32_t* bins = hist + seg * SEL_SEG * SEL_COLS + lane;
#pragma unroll
    for (int b = 0; b < SEL_SEG; ++b) {
      const uint32_t n = bins[b * SEL_COLS];
      if (!found) {
        if (rr <= n) {
          digit = (uint32_t)(seg * SEL_SEG + b);
          found = true;
        } else {
          rr -= n;
        }
      }
    }
    prefix = (prefix << 8) | digit;
    rank = found ? rr : 1u;
    __syncthreads();                                   // every wave has walked before the bins are cleared
  }
  if (bad && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && lane == 0) atomicOr(q.err_flag, TECM_BAD_GROUP);
  if (wave != 0 || !live) return;
  const float INF = std::numeric_limits<float>::infinity();
  q.out[((int64_t)qi * q.G + g) * q.C + c] = rank_in <= 0 ? -INF : (over ? INF : sel_value(prefix));
}

// ------------------------------------------------------------------------------------------------ (c)
__global__ __launch_bounds__(256) void interval_stats_kernel(TecmIntervalStats q) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.z;
  const int64_t i = (int64_t)blockIdx.x * CF_TILE + lane, h = (int64_t)blockIdx.y * CF_HC + wave;
  const bool own = i < q.I && h < q.H;       // this thread's cell is (g, h, i)
  const bool scaled = q.sigma != nullptr, score = q.target != nullptr;

  float qlo = 0.f, qhi = 0.f;
  if (own) {
    const int64_t cell = ((int64_t)(q.Gq == q.G ? g : 0) * q.H + h) * q.I + i;
    qhi = q.q_hi[cell];
    qlo = q.q_lo ? q.q_lo[cell] : -qhi;
  }
  const double pen = score ? 2.0 / q.alpha : 0.0;
  double a[TECM_INTERVAL_STATS];
#pragma unroll
  for (int n = 0; n < TECM_INTERVAL_STATS; ++n) a[n] = 0.0;

  bool present = false, bad = false;
  for (int64_t s0 = 0; s0 < q.S; s0 += CF_SB) {
    int match = 0;                           // block-uniform: which of the CF_SB samples belong to g
#pragma unroll
    for (int j = 0; j < CF_SB; ++j) {
      if (s0 + j < q.S) {
        const int id = q.group ? q.group[s0 + j] : 0;
        if (id == g) match |= 1 << j;
        if ((unsigned)id >= (unsigned)q.G) bad = true;
      }
    }
    if (!match) continue;
    present = true;
    if (!own) continue;
    float pv[CF_SB], tv[CF_SB], sv[CF_SB];
#pragma unroll
    for (int j = 0; j < CF_SB; ++j) {
      pv[j] = tv[j] = 0.f;
      sv[j] = 1.f;
      if (!(match >> j & 1)) continue;
      const int64_t s = s0 + j;
      pv[j] = q.pred[s * q.p_stride_s + h * q.p_stride_h + i * q.p_stride_i];
      if (score) tv[j] = q.target[s * q.t_stride_s + h * q.t_stride_h + i * q.t_stride_i];
      if (scaled) sv[j] = q.sigma[s * q.g_stride_s + h * q.g_stride_h + i * q.g_stride_i];
    }
#pragma unroll
    for (int j = 0; j < CF_SB; ++j) {        // ascending s
      if (!(match >> j & 1)) continue;
      float p, y;
      conformal_values(pv[j], tv[j], q.mean, q.scale, q.clip, q.clip_lo, q.clip_hi, p, y);
      const float w = scaled ? conformal_weight(sv[j], q.sigma_min) : 1.f;
      float lo = (float)((double)p + (double)qlo * (double)w), hi = (float)((double)p + (double)qhi * (double)w);
      if (q.clip) {
        lo = fminf(fmaxf(lo, q.clip_lo), q.clip_hi);
        hi = fminf(fmaxf(hi, q.clip_lo), q.clip_hi);
      }
      const int64_t o = (s0 + j) * q.o_stride_s + h * q.o_stride_h + i * q.o_stride_i;
      if (q.out_lo) q.out_lo[o] = lo;
      if (q.out_hi) q.out_hi[o] = hi;
      if (q.out_mid) q.out_mid[o] = p;
      if (!score) continue;
      const float r = conformal_score(p, y, q.mode, scaled, w);
      const bool cov = q.mode == TECM_CONF_ABS ? r <= qhi : (qlo <= r && r <= qhi);
      const bool below = !cov && (q.mode == TECM_CONF_ABS ? y < p : r < qlo);
      const double width = (double)hi - (double)lo, yd = y;
      const double wink = width + pen * fmax((double)lo - yd, 0.0) + pen * fmax(yd - (double)hi, 0.0);
      a[0] += 1.0;
      a[1] += cov ? 1.0 : 0.0;
      a[2] += below ? 1.0 : 0.0;
      a[3] += (!cov && !below) ? 1.0 : 0.0;
      a[4] += width;
      a[5] += wink;
    }
  }
  if (bad && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) atomicOr(q.err_flag, TECM_BAD_GROUP);
  if (!present || !own || !score) return;
  double* cell = q.stats + (((int64_t)g * q.H + h) * TECM_INTERVAL_STATS) * q.I + i;
#pragma unroll
  for (int n = 0; n < TECM_INTERVAL_STATS; ++n) cell[(int64_t)n * q.I] += a[n];
}

}  // namespace

extern "C" int tecm_conformal_scores(const TecmConformalScores* c, void* stream) {
  TECM_REQUIRE(c, TECM_E_ARG, "tecm_conformal_scores: null descriptor");
  TECM_REQUIRE(c->pred && c->target && c->scores, TECM_E_ARG, "tecm_conformal_scores: null pointer");
  TECM_REQUIRE(c->S > 0 && c->H > 0 && c->I > 0, TECM_E_ARG, "tecm_conformal_scores: bad shape");
  TECM_REQUIRE(c->mode == TECM_CONF_ABS || c->mode == TECM_CONF_SIGNED, TECM_E_ARG, "tecm_conformal_scores: unknown mode %d",
               (int)c->mode);
  TECM_REQUIRE(c->I <= INT64_MAX / (int64_t)sizeof(float) / c->H && c->ld >= (int64_t)c->H * c->I && c->row0 >= 0 &&
                   c->row0 + c->S <= INT64_MAX / (int64_t)sizeof(float) / c->ld,
               TECM_E_ARG, "tecm_conformal_scores: needs ld >= H * I, row0 >= 0 and a store within 64-bit addressing");
  TECM_REQUIRE(c->scale != 0.0, TECM_E_ARG, "tecm_conformal_scores: scale must be non-zero");
  TECM_REQUIRE(!c->sigma || c->sigma_min > 0.f, TECM_E_ARG, "tecm_conformal_scores: sigma needs sigma_min > 0");
  TECM_REQUIRE(tecm_aligned(c->pred, 4) && tecm_aligned(c->target, 4) && tecm_aligned(c->sigma, 4) && tecm_aligned(c->scores, 4),
               TECM_E_ALIGN, "tecm_conformal_scores: pred, target, sigma and scores must be 4-byte aligned");
  const int64_t chunks = ((int64_t)c->H + CF_HC - 1) / CF_HC, tiles = (c->I + CF_TILE - 1) / CF_TILE;
  TECM_REQUIRE(chunks <= 65535 && tiles < (1 << 24), TECM_E_ARG,
               "tecm_conformal_scores: ceil(H / 4) must be <= 65535 and ceil(I / 64) < 2^24");
  const unsigned zs = (unsigned)(c->S < 1024 ? c->S : 1024);
  hipLaunchKernelGGL(conformal_scores_kernel, dim3((unsigned)tiles, (unsigned)chunks, zs), dim3(256), 0, (hipStream_t)stream, *c);
  TECM_CHECK_LAUNCH("tecm_conformal_scores");
  return TECM_OK;
}

extern "C" int tecm_column_select(const TecmColumnSelect* c, void* stream) {
  TECM_REQUIRE(c, TECM_E_ARG, "tecm_column_select: null descriptor");
  TECM_REQUIRE(c->x && c->ranks && c->out && c->err_flag, TECM_E_ARG, "tecm_column_select: null pointer");
  TECM_REQUIRE(c->S > 0 && c->S < ((int64_t)1 << 31) && c->C > 0, TECM_E_ARG,
               "tecm_column_select: needs 0 < S < 2^31 and C > 0");
  TECM_REQUIRE(c->Q >= 1 && c->Q <= TECM_SELECT_MAX_Q, TECM_E_ARG, "tecm_column_select: Q = %d outside [1, %d]", (int)c->Q,
               TECM_SELECT_MAX_Q);
  TECM_REQUIRE(c->G >= 1 && c->G <= 65535, TECM_E_ARG, "tecm_column_select: G must lie in [1, 65535]");
  TECM_REQUIRE(c->ld >= c->C && c->ld <= INT64_MAX / (int64_t)sizeof(float) / c->S, TECM_E_ARG,
               "tecm_column_select: needs ld >= C and S * ld floats within 64-bit addressing");
  const int64_t tiles = (c->C + SEL_COLS - 1) / SEL_COLS;
  TECM_REQUIRE(tiles * c->G * c->Q < ((int64_t)1 << 31), TECM_E_ARG, "tecm_column_select: more than 2^31 blocks");
  TECM_REQUIRE(tecm_aligned(c->x, 4) && tecm_aligned(c->out, 4) && tecm_aligned(c->group, 4) && tecm_aligned(c->ranks, 4) &&
                   tecm_aligned(c->err_flag, 4),
               TECM_E_ALIGN, "tecm_column_select: x, out, group, ranks and err_flag must be 4-byte aligned");
  static bool attr_set = false;
  if (!attr_set) {
    TECM_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(&column_select_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEL_LDS) == hipSuccess,
                 TECM_E_LAUNCH, "tecm_column_select: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    attr_set = true;
  }
  hipLaunchKernelGGL(column_select_kernel, dim3((unsigned)tiles, (unsigned)c->G, (unsigned)c->Q), dim3(SEL_WAVES * 64), SEL_LDS,
                     (hipStream_t)stream, *c);
  TECM_CHECK_LAUNCH("tecm_column_select");
  return TECM_OK;
}

extern "C" int tecm_interval_stats(const TecmIntervalStats* c, void* stream) {
  TECM_REQUIRE(c, TECM_E_ARG, "tecm_interval_stats: null descriptor");
  TECM_REQUIRE(c->pred && c->q_hi && c->err_flag, TECM_E_ARG, "tecm_interval_stats: null pointer");
  TECM_REQUIRE(c->target ? c->stats != nullptr : (c->out_lo || c->out_hi || c->out_mid), TECM_E_ARG,
               "tecm_interval_stats: a target needs stats, no target needs a per-sample output");
  TECM_REQUIRE(c->S > 0 && c->H > 0 && c->I > 0 && c->G > 0, TECM_E_ARG, "tecm_interval_stats: bad shape");
  TECM_REQUIRE(c->mode == TECM_CONF_ABS || c->mode == TECM_CONF_SIGNED, TECM_E_ARG, "tecm_interval_stats: unknown mode %d",
               (int)c->mode);
  TECM_REQUIRE(c->mode == TECM_CONF_ABS || c->q_lo, TECM_E_ARG, "tecm_interval_stats: the signed mode needs q_lo");
  TECM_REQUIRE(c->Gq == 1 || c->Gq == c->G, TECM_E_ARG, "tecm_interval_stats: Gq must be 1 or G");
  TECM_REQUIRE(!c->target || (c->alpha > 0.0 && c->alpha < 1.0), TECM_E_ARG, "tecm_interval_stats: alpha must lie in (0, 1)");
  const int64_t chunks = ((int64_t)c->H + CF_HC - 1) / CF_HC, tiles = (c->I + CF_TILE - 1) / CF_TILE;
  TECM_REQUIRE(c->G <= 65535 && chunks <= 65535, TECM_E_ARG, "tecm_interval_stats: G and ceil(H / 4) must be <= 65535");
  TECM_REQUIRE(tiles < (1 << 24) && tiles * chunks < (1 << 24) && tiles * chunks * c->G < (1 << 24), TECM_E_ARG,
               "tecm_interval_stats: more than 2^24 blocks of 256 threads");
  TECM_REQUIRE(c->I <= INT64_MAX / (int64_t)sizeof(double) / TECM_INTERVAL_STATS / c->H / c->G, TECM_E_ARG,
               "tecm_interval_stats: G * H * 6 * I doubles do not fit 64-bit addressing");
  TECM_REQUIRE(c->scale != 0.0, TECM_E_ARG, "tecm_interval_stats: scale must be non-zero");
  TECM_REQUIRE(!c->sigma || c->sigma_min > 0.f, TECM_E_ARG, "tecm_interval_stats: sigma needs sigma_min > 0");
  TECM_REQUIRE(tecm_aligned(c->stats, 8) && tecm_aligned(c->group, 4) && tecm_aligned(c->err_flag, 4), TECM_E_ALIGN,
               "tecm_interval_stats: stats must be 8-byte aligned, group and err_flag 4-byte aligned");
  TECM_REQUIRE(tecm_aligned(c->pred, 4) && tecm_aligned(c->target, 4) && tecm_aligned(c->sigma, 4) && tecm_aligned(c->q_lo, 4) &&
                   tecm_aligned(c->q_hi, 4) && tecm_aligned(c->out_lo, 4) && tecm_aligned(c->out_hi, 4) &&
                   tecm_aligned(c->out_mid, 4),
               TECM_E_ALIGN, "tecm_interval_stats: operands, quantiles and per-sample outputs must be 4-byte aligned");
  hipLaunchKernelGGL(interval_stats_kernel, dim3((unsigned)tiles, (unsigned)chunks, (unsigned)c->G), dim3(256), 0,
                     (hipStream_t)stream, *c);
  TECM_CHECK_LAUNCH("tecm_interval_stats");
  return TECM_OK;
}
