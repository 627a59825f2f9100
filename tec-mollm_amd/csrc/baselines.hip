// Baseline forecasts for the evaluation of a test split (the second half of the reference's test.py and its
// src/models/baselines.py): per-window historical average / persistence / same-slot-one-period-ago straight from the
// device-resident series, and the per-node, per-slot mean that HistoricalAverage.fit computes.  Both are bandwidth work:
// one lane per node, the stride-C channel read touches whole 128-byte lines, no LDS tiling, no matrix cores.
#include "common.h"

namespace {

// ------------------------------------------------------------------ per-window baselines (test.py:46-71)
// One block per (window, tile of 256 nodes), the tiles of one window on consecutive blocks.  The arithmetic of MEAN is
// specified (tecmollm.h): sequential fp32 adds in ascending time order and one IEEE division.  Only the add order is fixed,
// so eight loads are issued ahead of the eight adds that consume them.
constexpr int WB_NODES = 256;
constexpr int WB_AHEAD = 8;

__global__ __launch_bounds__(WB_NODES) void window_baseline_kernel(TecmWindowBaseline w, int tiles) {
  const int b = blockIdx.x / tiles;
  const int n = (blockIdx.x - b * tiles) * WB_NODES + threadIdx.x;
  if (n >= w.N) return;
  const int64_t a = w.starts[b];
  float* o = w.out + (int64_t)b * w.o_stride_b + (int64_t)n * w.o_stride_n;
  const int reps = w.o_stride_h == 0 ? 1 : w.L_out;
  if (a < 0 || a + w.L_in > w.T) {                       // never read outside the series
    for (int h = 0; h < reps; ++h) o[h * w.o_stride_h] = __builtin_nanf("");
    return;
  }
  const int64_t row = (int64_t)w.N * w.C;
  const float* x = w.X + a * row + (int64_t)n * w.C + w.channel;
  if (w.mode == TECM_BASELINE_PERIODIC) {
    const float* xp = x + (int64_t)(w.L_in - w.period) * row;
    for (int h = 0; h < w.L_out; ++h) o[h * w.o_stride_h] = xp[(int64_t)(h % w.period) * row];
    return;
  }
  float val;
  if (w.mode == TECM_BASELINE_LAST) {
    val = x[(int64_t)(w.L_in - 1) * row];
  } else {
    float acc = x[0];
    int t = 1;
    for (; t + WB_AHEAD <= w.L_in; t += WB_AHEAD) {
      float v[WB_AHEAD];
#pragma unroll
      for (int j = 0; j < WB_AHEAD; ++j) v[j] = x[(int64_t)(t + j) * row];
#pragma unroll
      for (int j = 0; j < WB_AHEAD; ++j) acc += v[j];
    }
    for (; t < w.L_in; ++t) acc += x[(int64_t)t * row];
    val = __fdiv_rn(acc, (float)w.L_in);
  }
  for (int h = 0; h < reps; ++h) o[h * w.o_stride_h] = val;
}

// ------------------------------------------------------------------ HistoricalAverage.fit (baselines.py:13-33)
// One block per (tile of 64 nodes, slot): lane = node, each of the four waves walks one quarter of T in ascending order
// and adds the rows of its slot in fp64; the quarters meet in LDS in a fixed order.  The slot of a time step is the same for
// the whole wave, so a row that belongs to another slot is never loaded: every element of the series is read once.
constexpr int SM_NODES = 64;

__global__ __launch_bounds__(256) void slot_mean_kernel(TecmSlotMean m) {
  __shared__ double part[4][SM_NODES];
  __shared__ double cnt[4];
  const int s = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = blockIdx.x * SM_NODES + lane;
  const bool live = n < m.N;
  const float* x = m.x + (int64_t)(live ? n : 0) * m.stride_n;
  const int64_t per = (m.T + 3) >> 2;
  const int64_t t0 = q * per;
  const int64_t t1 = t0 + per < m.T ? t0 + per : m.T;
  double acc = 0.0, c = 0.0;
  for (int64_t t = t0; t < t1; ++t) {
    if (m.slot[t] == s) {
      c += 1.0;
      if (live) acc += (double)x[t * m.stride_t];
    }
  }
  part[q][lane] = acc;
  if (lane == 0) cnt[q] = c;
  __syncthreads();
  if (q == 0) {
    const double sum = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    const double count = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
    if (live) m.means[(int64_t)n * m.n_slots + s] = sum / count;          // 0 / 0 = NaN for an empty slot
    if (blockIdx.x == 0 && lane == 0) m.counts[s] = count;
  }
}

}  // namespace

extern "C" int tecm_window_baseline(const TecmWindowBaseline* w, void* stream) {
  TECM_REQUIRE(w, TECM_E_ARG, "tecm_window_baseline: null descriptor");
  TECM_REQUIRE(w->X && w->starts && w->out, TECM_E_ARG, "tecm_window_baseline: null pointer");
  TECM_REQUIRE(w->T > 0 && w->N > 0 && w->C > 0 && w->L_in > 0 && w->L_out > 0 && w->B > 0 && w->L_in <= w->T, TECM_E_ARG,
               "tecm_window_baseline: bad shape");
  TECM_REQUIRE(w->channel >= 0 && w->channel < w->C, TECM_E_ARG, "tecm_window_baseline: channel %d outside [0, %d)",
               w->channel, w->C);
  TECM_REQUIRE(w->mode == TECM_BASELINE_MEAN || w->mode == TECM_BASELINE_LAST || w->mode == TECM_BASELINE_PERIODIC,
               TECM_E_ARG, "tecm_window_baseline: unknown mode %d", w->mode);
  TECM_REQUIRE(w->mode != TECM_BASELINE_PERIODIC || (w->period > 0 && w->period <= w->L_in), TECM_E_ARG,
               "tecm_window_baseline: PERIODIC needs 0 < period <= L_in (period %d, L_in %d)", w->period, w->L_in);
  TECM_REQUIRE(w->mode != TECM_BASELINE_PERIODIC || w->L_out == 1 || w->o_stride_h != 0, TECM_E_ARG,
               "tecm_window_baseline: PERIODIC differs per horizon and needs a non-zero horizon stride");
  if (w->starts_host_check) {
    for (int b = 0; b < w->B; ++b) {
      const int64_t a = w->starts_host_check[b];
      TECM_REQUIRE(a >= 0 && a + w->L_in <= w->T, TECM_E_ARG,
                   "tecm_window_baseline: window %d starts at %lld, outside [0, T - L_in]", b, (long long)a);
    }
  }
  const int tiles = (w->N + WB_NODES - 1) / WB_NODES;
  TECM_REQUIRE((int64_t)tiles * w->B <= 0x7fffffffLL, TECM_E_ARG, "tecm_window_baseline: too many windows for one launch");
  hipLaunchKernelGGL(window_baseline_kernel, dim3((unsigned)(tiles * w->B)), dim3(WB_NODES), 0, (hipStream_t)stream, *w, tiles);
  TECM_CHECK_LAUNCH("tecm_window_baseline");
  return TECM_OK;
}

extern "C" int tecm_slot_mean(const TecmSlotMean* m, void* stream) {
  TECM_REQUIRE(m, TECM_E_ARG, "tecm_slot_mean: null descriptor");
  TECM_REQUIRE(m->x && m->slot && m->means && m->counts, TECM_E_ARG, "tecm_slot_mean: null pointer");
  TECM_REQUIRE(m->T > 0 && m->N > 0 && m->n_slots > 0 && m->n_slots <= 65535, TECM_E_ARG,
               "tecm_slot_mean: bad shape (0 < n_slots <= 65535)");
  TECM_REQUIRE(m->stride_t >= 0 && m->stride_n >= 0, TECM_E_ARG, "tecm_slot_mean: negative stride");
  TECM_REQUIRE(tecm_aligned(m->means, 8) && tecm_aligned(m->counts, 8), TECM_E_ALIGN,
               "tecm_slot_mean: means and counts must be 8-byte aligned");
  hipLaunchKernelGGL(slot_mean_kernel, dim3((m->N + SM_NODES - 1) / SM_NODES, m->n_slots), dim3(256), 0,
                     (hipStream_t)stream, *m);
  TECM_CHECK_LAUNCH("tecm_slot_mean");
  return TECM_OK;
}
