// Evaluation statistics per cell (group, horizon, node): tecm_metrics_map (include/tecmollm.h (3b)), the kernel under
// MapMetrics (src/evaluation/metrics.py) -- error maps and storm- / time-of-day-stratified scores without a host copy of the
// predictions.  A streaming kernel: a few MB per update, no matrix cores.
//
// Block (x, y, z) = (tile of 64 nodes, chunk of 4 horizons, group g), 256 threads: lane = node of the tile, wave w owns
// horizon h0 + w, so a thread owns ONE cell and keeps its 8 sums in registers.  It walks the samples in ascending s,
// sixteen at a time so that the loads of a whole batch of 16 are in flight together, takes those whose group is g, and adds
// its sums to `stats` once at the end: one owner per cell, no atomics, a fixed order.  A block whose group does not occur
// among the S ids touches no statistics.  (Twelve horizons per block and four samples in flight, the first cut, left 46
// blocks walking four dependent rounds at N = 2911, B = 16, G = 1 and took 34 us for 9 MB; this shape takes 18 us,
// profiles/error_maps.txt.  Either way the kernel is bound by its chain of memory latencies and its launch, not by bytes.)
//
// An operand whose nodes are contiguous (stride_i == 1) is read in place: a wave reads 64 consecutive floats per horizon.
// The model's output is the permuted view with stride_h == 1, stride_i == H: 64 nodes x H horizons are 64*H contiguous floats.
// There the chunk's 4 columns of the tile's 64 rows are staged in LDS -- 16 contiguous bytes per row and lane quad, 16 rows
// per wave instruction instead of 64 -- in rows padded to 5 floats (odd pitch: the column reads of 64 lanes fall on distinct
// banks; window_y_kernel's L_out + 1) and read back node per lane.
// H limit of the LDS path, TECM_MAP_LDS_MAX_H = 32: up to there a row of the slab is at most one 128-B cache line and the
// staging pulls every line of the slab once per chunk block, in 16-B pieces.  Past it every 16-B piece lies in a line of its
// own, which is also what the four waves of a block touch when they read their four neighbouring floats in place, so the
// staging and its barriers buy nothing; larger H is read in place.  The forecast lengths in use are 12 and 24.
#include "common.h"
#include "metrics_value.h"

namespace {

constexpr int MAP_TILE = 64;                 // nodes per block = lanes of a wave
constexpr int MAP_HC = 4;                    // horizons per block = waves
constexpr int MAP_LD = MAP_HC + 1;           // padded LDS row
constexpr int MAP_SB = 16;                   // samples in flight
constexpr int MAP_SLAB = MAP_SB * MAP_TILE * MAP_LD;     // floats of LDS per staged operand (20 KiB)

// the chunk's columns of the tile's rows of one sample: base[(i0 + r)*H + h0 + c] -> slab[r*MAP_LD + c]
__device__ __forceinline__ void stage(float* slab, const float* base, int64_t H, int h0, int hc, int cnt) {
  for (int e = threadIdx.x; e < cnt * hc; e += 256) {
    const int r = e / hc, c = e - r * hc;
    slab[r * MAP_LD + c] = base[(int64_t)r * H + h0 + c];
  }
}

__global__ __launch_bounds__(256) void metrics_map_kernel(TecmMetricsMap q, int p_lds, int t_lds) {
  extern __shared__ float slab[];            // [pred if p_lds][target if t_lds], MAP_SLAB floats each
  float* slab_p = slab;
  float* slab_t = slab + (p_lds ? MAP_SLAB : 0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.z;
  const int h0 = blockIdx.y * MAP_HC;
  const int hc = min(MAP_HC, q.H - h0);
  const int64_t i0 = (int64_t)blockIdx.x * MAP_TILE;
  const int cnt = (int)(q.I - i0 < MAP_TILE ? q.I - i0 : MAP_TILE);
  const int64_t i = i0 + lane, h = h0 + wave;
  const bool own = lane < cnt && wave < hc;  // this thread's cell is (g, h, i)

  double a[TECM_METRIC_STATS];
#pragma unroll
  for (int n = 0; n < TECM_METRIC_STATS; ++n) a[n] = 0.0;

  bool present = false, bad = false;
  for (int64_t s0 = 0; s0 < q.S; s0 += MAP_SB) {
    int match = 0;                           // block-uniform: which of the MAP_SB samples belong to g
#pragma unroll
    for (int j = 0; j < MAP_SB; ++j) {
      if (s0 + j < q.S) {
        const int id = q.group ? q.group[s0 + j] : 0;
        if (id == g) match |= 1 << j;
        if ((unsigned)id >= (unsigned)q.G) bad = true;
      }
    }
    if (!match) continue;
    present = true;
    float pv[MAP_SB], tv[MAP_SB];
#pragma unroll
    for (int j = 0; j < MAP_SB; ++j) {       // operands read in place first: in flight while the other one is staged
      pv[j] = tv[j] = 0.f;
      if (!(match >> j & 1) || !own) continue;
      const int64_t s = s0 + j;
      if (!p_lds) pv[j] = q.pred[s * q.p_stride_s + h * q.p_stride_h + i * q.p_stride_i];
      if (!t_lds) tv[j] = q.target[s * q.t_stride_s + h * q.t_stride_h + i * q.t_stride_i];
    }
    if (p_lds || t_lds) {
#pragma unroll
      for (int j = 0; j < MAP_SB; ++j) {
        if (!(match >> j & 1)) continue;
        if (p_lds) stage(slab_p + j * MAP_TILE * MAP_LD, q.pred + (s0 + j) * q.p_stride_s + i0 * q.H, q.H, h0, hc, cnt);
        if (t_lds) stage(slab_t + j * MAP_TILE * MAP_LD, q.target + (s0 + j) * q.t_stride_s + i0 * q.H, q.H, h0, hc, cnt);
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < MAP_SB; ++j) {
        if (!(match >> j & 1) || !own) continue;
        if (p_lds) pv[j] = slab_p[(j * MAP_TILE + lane) * MAP_LD + wave];
        if (t_lds) tv[j] = slab_t[(j * MAP_TILE + lane) * MAP_LD + wave];
      }
    }
#pragma unroll
    for (int j = 0; j < MAP_SB; ++j) {       // ascending s
      if (!(match >> j & 1) || !own) continue;
      float p32 = pv[j], t32 = tv[j];
      if (!isfinite(p32)) p32 = 0.f;                                       // metrics.py:139-145
      p32 = nan_to_num_tec(unscale_f32(p32, q.mean, q.scale));             // :36-46
      t32 = nan_to_num_tec(unscale_f32(t32, q.mean, q.scale));
      if (q.clip) p32 = fminf(fmaxf(p32, q.clip_lo), q.clip_hi);           // :50-51
      const double t = t32, p = p32, d = t - p;
      a[0] += 1.0; a[1] += t; a[2] += p; a[3] += t * t; a[4] += p * p; a[5] += t * p; a[6] += fabs(d); a[7] += d * d;
    }
    if (p_lds || t_lds) __syncthreads();     // the tile is overwritten by the next MAP_SB samples
  }
  if (bad && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) atomicOr(q.err_flag, TECM_BAD_GROUP);
  if (!present || !own) return;
  double* cell = q.stats + (((int64_t)g * q.H + h) * TECM_METRIC_STATS) * q.I + i;
#pragma unroll
  for (int n = 0; n < TECM_METRIC_STATS; ++n) cell[(int64_t)n * q.I] += a[n];
}

}  // namespace

extern "C" int tecm_metrics_map(const TecmMetricsMap* m, void* stream) {
  TECM_REQUIRE(m, TECM_E_ARG, "tecm_metrics_map: null descriptor");
  TECM_REQUIRE(m->pred && m->target && m->stats && m->err_flag, TECM_E_ARG, "tecm_metrics_map: null pointer");
  TECM_REQUIRE(m->S > 0 && m->H > 0 && m->I > 0 && m->G > 0, TECM_E_ARG, "tecm_metrics_map: bad shape");
  const int64_t chunks = ((int64_t)m->H + MAP_HC - 1) / MAP_HC, tiles = (m->I + MAP_TILE - 1) / MAP_TILE;
  TECM_REQUIRE(m->G <= 65535 && chunks <= 65535, TECM_E_ARG,
               "tecm_metrics_map: G and ceil(H / 4) must be <= 65535");
  TECM_REQUIRE(tiles < (1 << 24) && tiles * chunks < (1 << 24) && tiles * chunks * m->G < (1 << 24), TECM_E_ARG,
               "tecm_metrics_map: more than 2^24 blocks of 256 threads");
  TECM_REQUIRE(m->I <= INT64_MAX / (int64_t)sizeof(double) / TECM_METRIC_STATS / m->H / m->G, TECM_E_ARG,
               "tecm_metrics_map: G * H * 8 * I doubles do not fit 64-bit addressing");
  TECM_REQUIRE(m->scale != 0.0, TECM_E_ARG, "tecm_metrics_map: scale must be non-zero");
  TECM_REQUIRE(tecm_aligned(m->stats, 8) && tecm_aligned(m->group, 4) && tecm_aligned(m->err_flag, 4), TECM_E_ALIGN,
               "tecm_metrics_map: stats must be 8-byte aligned, group and err_flag 4-byte aligned");
  const bool lds_h = m->H > 1 && m->H <= TECM_MAP_LDS_MAX_H && m->I > 1;
  const int p_lds = lds_h && m->p_stride_h == 1 && m->p_stride_i == m->H;
  const int t_lds = lds_h && m->t_stride_h == 1 && m->t_stride_i == m->H;
  const size_t lds = (size_t)(p_lds + t_lds) * MAP_SLAB * sizeof(float);
  hipLaunchKernelGGL(metrics_map_kernel, dim3((unsigned)tiles, (unsigned)chunks, (unsigned)m->G), dim3(256), lds,
                     (hipStream_t)stream, *m, p_lds, t_lds);
  TECM_CHECK_LAUNCH("tecm_metrics_map");
  return TECM_OK;
}
