// Significance of the comparison: the statistics of every WINDOW kept apart (tecm_metrics_window) and paired circular
// block-bootstrap sums over them (tecm_block_bootstrap); include/tecmollm.h (3h).  Under tecmollm/significance.py:
// confidence intervals of every metric and of the improvement percentages, and the Diebold-Mariano test.  Streaming
// kernels, float64 additions only, no atomics on any sum: both are restated addition by addition in
// tests/significance_ref.py.
//
// (a) metrics_window_kernel.  Block (x, y) = (sample s, chunk of 4 horizons), 256 threads: wave w owns horizon h0 + w of
// sample s, lane l owns the nodes i = 64*k + l.  SUMMATION ORDER of one (s, h), for each of the eight statistics:
//   1. lane l adds its terms in ascending tile k = 0, 1, ... into a partial that starts at +0.0 (a lane without a node
//      keeps +0.0);
//   2. the 64 partials are joined by a butterfly: for o = 32, 16, 8, 4, 2, 1: partial[l] += partial[l ^ o].  IEEE addition
//      commutes, so every lane ends with the same bits: ((p[0..31] + p[32..63]) halves again and again down to one value.
// The (t, p) pipeline is metrics_map_kernel's (metrics_value.h plus the non-finite guard and the clip).  A row of the table
// is OVERWRITTEN by the one wave that owns it; rows that no sample names are not touched.  A row index outside
// [0, table_rows) writes nothing and sets TECM_BAD_ROW.
// Operands: node-contiguous ones (stride_i == 1; stride_h may be 0) are read in place, 64 consecutive floats per wave.  The
// model's view (stride_h == 1, stride_i == H) is staged as in metrics_map.hip: the chunk's 4 columns of a tile's 64 rows are
// 16 contiguous bytes per row, pulled by lane quads into LDS rows padded to 5 floats and read back node per lane; same H
// limit (TECM_MAP_LDS_MAX_H) for the same reason.  Eight tiles are in flight per round.
//
// (b) block_bootstrap_kernel.  Block (x, y) = (replicate r, (forecast m, group g, 64-wide chunk of W)), ONE wave: lane =
// column, so a lane owns one output value and a table row is one coalesced read (768 B at W = 96 over two blocks).  The
// wave walks the positions t = 0 .. S-1 in ascending order, sixteen at a time: the window of position t = k*L + j is
// (starts[r, k] + j) mod S, all wave-uniform; rows whose group is not g are not loaded; the sixteen loads are issued
// together, then added to ONE running float64 sum in ascending t.  No LDS, no join.
#include "common.h"
#include "metrics_value.h"

namespace {

constexpr int WIN_TILE = 64;                 // nodes per tile = lanes of a wave
constexpr int WIN_HC = 4;                    // horizons per block = waves
constexpr int WIN_LD = WIN_HC + 1;           // padded LDS row
constexpr int WIN_TB = 8;                    // tiles in flight
constexpr int WIN_SLAB = WIN_TB * WIN_TILE * WIN_LD;     // floats of LDS per staged operand (10 KiB)

// the chunk's columns of the tile's rows: base[r*H + h0 + c] -> slab[r*WIN_LD + c]
__device__ __forceinline__ void stage(float* slab, const float* base, int64_t H, int h0, int hc, int cnt) {
  for (int e = threadIdx.x; e < cnt * hc; e += 256) {
    const int r = e / hc, c = e - r * hc;
    slab[r * WIN_LD + c] = base[(int64_t)r * H + h0 + c];
  }
}

__global__ __launch_bounds__(256) void metrics_window_kernel(TecmMetricsWindow q, int p_lds, int t_lds) {
  extern __shared__ float slab[];            // [pred if p_lds][target if t_lds], WIN_SLAB floats each
  float* slab_p = slab;
  float* slab_t = slab + (p_lds ? WIN_SLAB : 0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s = blockIdx.x;
  const int h0 = blockIdx.y * WIN_HC;
  const int hc = min(WIN_HC, q.H - h0);
  const int64_t h = h0 + wave;
  const int64_t row = q.rows ? q.rows[s] : q.row0 + s;
  if (row < 0 || row >= q.table_rows) {      // block-uniform, before any barrier
    if (blockIdx.y == 0 && threadIdx.x == 0) atomicOr(q.err_flag, TECM_BAD_ROW);
    return;
  }
  const float* pred = q.pred + s * q.p_stride_s;
  const float* target = q.target + s * q.t_stride_s;

  double a[TECM_METRIC_STATS];
#pragma unroll
  for (int n = 0; n < TECM_METRIC_STATS; ++n) a[n] = 0.0;

  const int64_t ntiles = (q.I + WIN_TILE - 1) / WIN_TILE;
  for (int64_t k0 = 0; k0 < ntiles; k0 += WIN_TB) {
    float pv[WIN_TB], tv[WIN_TB];
#pragma unroll
    for (int j = 0; j < WIN_TB; ++j) {       // operands read in place first: in flight while the other one is staged
      pv[j] = tv[j] = 0.f;
      const int64_t i = (k0 + j) * WIN_TILE + lane;
      if (i >= q.I || wave >= hc) continue;
      if (!p_lds) pv[j] = pred[h * q.p_stride_h + i * q.p_stride_i];
      if (!t_lds) tv[j] = target[h * q.t_stride_h + i * q.t_stride_i];
    }
    if (p_lds || t_lds) {
#pragma unroll
      for (int j = 0; j < WIN_TB; ++j) {
        const int64_t i0 = (k0 + j) * WIN_TILE;
        if (i0 >= q.I) continue;
        const int cnt = (int)(q.I - i0 < WIN_TILE ? q.I - i0 : WIN_TILE);
        if (p_lds) stage(slab_p + j * WIN_TILE * WIN_LD, pred + i0 * q.H, q.H, h0, hc, cnt);
        if (t_lds) stage(slab_t + j * WIN_TILE * WIN_LD, target + i0 * q.H, q.H, h0, hc, cnt);
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < WIN_TB; ++j) {
        if ((k0 + j) * WIN_TILE + lane >= q.I || wave >= hc) continue;
        if (p_lds) pv[j] = slab_p[(j * WIN_TILE + lane) * WIN_LD + wave];
        if (t_lds) tv[j] = slab_t[(j * WIN_TILE + lane) * WIN_LD + wave];
      }
    }
#pragma unroll
    for (int j = 0; j < WIN_TB; ++j) {       // ascending tile
      if ((k0 + j) * WIN_TILE + lane >= q.I || wave >= hc) continue;
      float p32 = pv[j], t32 = tv[j];
      if (!isfinite(p32)) p32 = 0.f;                                       // metrics.py:139-145
      p32 = nan_to_num_tec(unscale_f32(p32, q.mean, q.scale));             // :36-46
      t32 = nan_to_num_tec(unscale_f32(t32, q.mean, q.scale));
      if (q.clip) p32 = fminf(fmaxf(p32, q.clip_lo), q.clip_hi);           // :50-51
      const double t = t32, p = p32, d = t - p;
      a[0] += 1.0; a[1] += t; a[2] += p; a[3] += t * t; a[4] += p * p; a[5] += t * p; a[6] += fabs(d); a[7] += d * d;
    }
    if (p_lds || t_lds) __syncthreads();     // the slab is overwritten by the next WIN_TB tiles
  }
  double mine = 0.0;                          // lane n < 8 keeps statistic n: one 64-byte store per (s, h)
#pragma unroll
  for (int n = 0; n < TECM_METRIC_STATS; ++n) {
    double v = a[n];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == n) mine = v;
  }
  if (wave < hc && lane < TECM_METRIC_STATS) q.table[(row * q.H + h) * TECM_METRIC_STATS + lane] = mine;
}

constexpr int BOOT_TB = 16;                  // positions (row loads) in flight

__global__ __launch_bounds__(64) void block_bootstrap_kernel(TecmBlockBootstrap q, int wchunks) {
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  int rest = blockIdx.y;
  const int chunk = rest % wchunks; rest /= wchunks;
  const int g = rest % q.G;
  const int m = rest / q.G;
  const int64_t w = (int64_t)chunk * 64 + lane;
  const bool own = w < q.W;
  const double* col = q.table + (int64_t)m * q.stride_m + (own ? w : 0);
  const int32_t* starts = q.starts + r * q.K;
  const int S = (int)q.S, L = (int)q.L;

  double acc = 0.0;
  bool bad_start = false, bad_group = false;
  int k = 0, j = 0;                          // position t = k*L + j
  for (int t0 = 0; t0 < S; t0 += BOOT_TB) {
    double v[BOOT_TB];
    unsigned take = 0;                       // wave-uniform: which of the BOOT_TB positions belong to g
#pragma unroll
    for (int u = 0; u < BOOT_TB; ++u) {
      v[u] = 0.0;
      if (t0 + u < S) {
        const int st = starts[k];
        if (st < 0 || st >= S) {
          bad_start = true;
        } else {
          int64_t row = (int64_t)st + j;     // j <= t < S: one wrap at most
          if (row >= S) row -= S;
          const int id = q.group ? q.group[row] : 0;
          if (id < 0 || id >= q.G) bad_group = true;
          else if (id == g) {
            take |= 1u << u;
            if (own) v[u] = col[row * q.stride_s];
          }
        }
        if (++j == L) { j = 0; ++k; }
      }
    }
#pragma unroll
    for (int u = 0; u < BOOT_TB; ++u)        // ascending t
      if (take >> u & 1) acc += v[u];
  }
  if (blockIdx.y == 0 && lane == 0) {
    if (bad_start) atomicOr(q.err_flag, TECM_BAD_START);
    if (bad_group) atomicOr(q.err_flag, TECM_BAD_GROUP);
  }
  if (own) q.out[((r * q.M + m) * q.G + g) * q.W + w] = acc;
}

}  // namespace

extern "C" int tecm_metrics_window(const TecmMetricsWindow* m, void* stream) {
  TECM_REQUIRE(m, TECM_E_ARG, "tecm_metrics_window: null descriptor");
  TECM_REQUIRE(m->pred && m->target && m->table && m->err_flag, TECM_E_ARG, "tecm_metrics_window: null pointer");
  TECM_REQUIRE(m->S > 0 && m->H > 0 && m->I > 0 && m->table_rows > 0, TECM_E_ARG, "tecm_metrics_window: bad shape");
  const int64_t chunks = ((int64_t)m->H + WIN_HC - 1) / WIN_HC;
  TECM_REQUIRE(m->S < ((int64_t)1 << 31) && chunks <= 65535, TECM_E_ARG,
               "tecm_metrics_window: S must be < 2^31 and ceil(H / 4) <= 65535");
  TECM_REQUIRE(m->table_rows <= INT64_MAX / (int64_t)sizeof(double) / TECM_METRIC_STATS / m->H, TECM_E_ARG,
               "tecm_metrics_window: table_rows * H * 8 doubles do not fit 64-bit addressing");
  TECM_REQUIRE(m->scale != 0.0, TECM_E_ARG, "tecm_metrics_window: scale must be non-zero");
  TECM_REQUIRE(tecm_aligned(m->table, 8) && tecm_aligned(m->rows, 8) && tecm_aligned(m->err_flag, 4) &&
                   tecm_aligned(m->pred, 4) && tecm_aligned(m->target, 4),
               TECM_E_ALIGN, "tecm_metrics_window: table and rows must be 8-byte aligned, pred, target and err_flag 4-byte aligned");
  const bool lds_h = m->H > 1 && m->H <= TECM_MAP_LDS_MAX_H && m->I > 1;
  const int p_lds = lds_h && m->p_stride_h == 1 && m->p_stride_i == m->H;
  const int t_lds = lds_h && m->t_stride_h == 1 && m->t_stride_i == m->H;
  const size_t lds = (size_t)(p_lds + t_lds) * WIN_SLAB * sizeof(float);
  hipLaunchKernelGGL(metrics_window_kernel, dim3((unsigned)m->S, (unsigned)chunks), dim3(256), lds, (hipStream_t)stream, *m,
                     p_lds, t_lds);
  TECM_CHECK_LAUNCH("tecm_metrics_window");
  return TECM_OK;
}

extern "C" int tecm_block_bootstrap(const TecmBlockBootstrap* b, void* stream) {
  TECM_REQUIRE(b, TECM_E_ARG, "tecm_block_bootstrap: null descriptor");
  TECM_REQUIRE(b->table && b->starts && b->out && b->err_flag, TECM_E_ARG, "tecm_block_bootstrap: null pointer");
  TECM_REQUIRE(b->M > 0 && b->W > 0 && b->R > 0, TECM_E_ARG, "tecm_block_bootstrap: bad shape");
  TECM_REQUIRE(b->S > 0 && b->S < ((int64_t)1 << 31) && b->R < ((int64_t)1 << 31), TECM_E_ARG,
               "tecm_block_bootstrap: need 0 < S < 2^31 and R < 2^31");
  TECM_REQUIRE(b->L >= 1 && b->L < ((int64_t)1 << 31), TECM_E_ARG, "tecm_block_bootstrap: need 1 <= block_len < 2^31");
  TECM_REQUIRE(b->K == (b->S + b->L - 1) / b->L, TECM_E_ARG, "tecm_block_bootstrap: K must be ceil(S / block_len)");
  TECM_REQUIRE(b->G >= 1 && b->G <= 65535, TECM_E_ARG, "tecm_block_bootstrap: G outside [1, 65535]");
  const int64_t wchunks = (b->W + 63) / 64;
  TECM_REQUIRE(b->W < ((int64_t)1 << 31) && wchunks * b->G <= 65535 && wchunks * b->G * b->M <= 65535, TECM_E_ARG,
               "tecm_block_bootstrap: M * G * ceil(W / 64) must be <= 65535");
  TECM_REQUIRE(b->stride_s >= b->W && b->stride_m >= 0, TECM_E_ARG,
               "tecm_block_bootstrap: need stride_s >= W (rows W-contiguous) and stride_m >= 0");
  TECM_REQUIRE(b->R <= INT64_MAX / (int64_t)sizeof(double) / b->M / b->G / b->W, TECM_E_ARG,
               "tecm_block_bootstrap: R * M * G * W doubles do not fit 64-bit addressing");
  TECM_REQUIRE(tecm_aligned(b->table, 8) && tecm_aligned(b->out, 8) && tecm_aligned(b->starts, 4) &&
                   tecm_aligned(b->group, 4) && tecm_aligned(b->err_flag, 4),
               TECM_E_ALIGN, "tecm_block_bootstrap: table and out must be 8-byte aligned, starts, group and err_flag 4-byte aligned");
  hipLaunchKernelGGL(block_bootstrap_kernel, dim3((unsigned)b->R, (unsigned)(wchunks * b->G * b->M)), dim3(64), 0,
                     (hipStream_t)stream, *b, (int)wchunks);
  TECM_CHECK_LAUNCH("tecm_block_bootstrap");
  return TECM_OK;
}
