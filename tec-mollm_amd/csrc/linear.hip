// LinearBaseline (tecmollm.h (9)) on the device: the normal equations of a per-node ridge regression from the input window to
// the H targets, accumulated over every window of a split (lin_gram_kernel, the hot path), their Cholesky solve
// (lin_solve_kernel) and the forecast of any number of windows in one launch (lin_forecast_kernel).  All arithmetic is fp64.
//
// Gram geometry.  Per-node sums want time-major data and the split is (T, N, C), so a block owns a tile of nodes for the WHOLE
// series and walks it in chunks of windows.  A chunk is staged in LDS as doubles, [channel | ys][node][t], with a halo of the
// largest look-back plus H rows, next to one region of ones that serves the intercept and every padded row or column.  A lane
// owns an 8 x 4 sub-rectangle of a node's P x (P+H) array [G | R], rows rg + RG k and columns cg + CG m, so that the lanes of
// one read instruction touch consecutive lags: consecutive LDS doubles.  Per window a lane issues 12 LDS reads for 32 FMAs
// and keeps its 32 accumulators in registers from the first window to the last: every entry is one chain in ascending window
// order.  (A wave-per-16-rows split with broadcast row reads needs 17 reads per 16 or 32 FMAs and is bound by the LDS issue
// rate on the default P + H = 61; this one keeps the LDS under the fp64 FMA time.)  Measured at T = 4380, N = 2911, P = 49,
// H = 12 (profiles/linear.txt): what binds is the issue slots of the 12 reads and their address updates beside the 32 FMAs,
// so the stride-1 loop makes four windows per trip through the same 12 addresses, and the registers are capped at 128 for
// four waves per SIMD -- 2.94 ms as first written (166 registers, three waves), 2.35 ms capped, 1.98 ms with both.
#include "common.h"

namespace {

constexpr int LG_RT = 8, LG_CT = 4;                       // rows and columns of [G | R] per lane
constexpr int LG_MAX_TILE = 4;                             // nodes per block
constexpr int LG_MAX_THREADS = 768;                        // 4 nodes x 8 row groups x 24 column groups
constexpr int LG_LDS_DOUBLES = 8192;                       // 64 KiB
constexpr int LG_WAVES = 4;                                // per SIMD: at most 128 registers, two 7-wave blocks of the default shape per CU
constexpr int LG_UNROLL = 4;                               // windows per trip of the stride-1 loop
constexpr int LIN_P = TECM_LIN_MAX_P, LIN_H = TECM_LIN_MAX_H;

struct LinGramArgs {
  TecmLinGram g;
  int32_t slot[LIN_P];                 // predictor p reads staged channel slot[p]
  int32_t chans[TECM_LIN_MAX_CHANNELS];
  int32_t nch, maxlag, tile, chunk, S, RG, CG, threads;
};

template <bool UNIT>
__global__ __launch_bounds__(LG_MAX_THREADS, LG_WAVES) void lin_gram_kernel(LinGramArgs a) {
  extern __shared__ double lg_lds[];
  const TecmLinGram& g = a.g;
  const int P = g.P, H = g.H, S = a.S, tile = a.tile, nslots = a.nch + 1;
  const int lpn = a.RG * a.CG;
  const int tid = threadIdx.x;
  const int nl = tid / lpn, q = tid - nl * lpn;
  const int rg = q / a.CG, cg = q - rg * a.CG;
  const int64_t n0 = (int64_t)blockIdx.x * tile;
  const bool worker = nl < tile;                           // the lanes that round the block up to whole waves only stage
  const int ones = tile * nslots * S;
  // LDS offset, at the chunk's first window, of column j of [z | y]
  auto column = [&](int j) {
    if (!worker || j <= 0 || j >= P + H) return ones;
    if (j < P) return (a.slot[j] * tile + nl) * S + a.maxlag - g.lag[j];
    return (a.nch * tile + nl) * S + a.maxlag + (j - P);
  };
  int roff[LG_RT], coff[LG_CT];
#pragma unroll
  for (int k = 0; k < LG_RT; ++k) roff[k] = rg + a.RG * k < P ? column(rg + a.RG * k) : ones;
#pragma unroll
  for (int m = 0; m < LG_CT; ++m) coff[m] = column(cg + a.CG * m);
  double acc[LG_RT][LG_CT];
#pragma unroll
  for (int k = 0; k < LG_RT; ++k)
#pragma unroll
    for (int m = 0; m < LG_CT; ++m) acc[k][m] = 0.0;
  for (int t = tid; t < S; t += a.threads) lg_lds[ones + t] = 1.0;

  const int step = (int)g.step;
  const int64_t row = (int64_t)g.N * g.C;
  for (int64_t w0 = 0; w0 < g.count; w0 += a.chunk) {
    const int wc = g.count - w0 < a.chunk ? (int)(g.count - w0) : a.chunk;
    const int64_t t0 = g.first + w0 * g.step + g.L_in - a.maxlag;          // the series row of LDS slot 0
    const int rows = (wc - 1) * step + a.maxlag + H;                        // <= S
    __syncthreads();                                                       // the previous chunk has been consumed
    const int per_t = tile * nslots;
    for (int e = tid; e < rows * per_t; e += a.threads) {
      const int t = e / per_t, r = e - t * per_t;
      const int nloc = r / nslots, s = r - nloc * nslots;
      const int64_t tt = t0 + t, n = n0 + nloc;
      double v = 0.0;
      if (n < g.N) {
        if (s < a.nch) {
          if (tt < g.T) v = (double)g.X[tt * row + n * g.C + a.chans[s]];
        } else if (tt < g.Ty) {
          v = (double)g.ys[tt * g.ys_stride_t + n * g.ys_stride_n];
        }
      }
      lg_lds[(s * tile + nloc) * S + t] = v;
    }
    __syncthreads();
    if (worker) {
      auto window = [&](int o) {
        double zr[LG_RT], zc[LG_CT];
#pragma unroll
        for (int k = 0; k < LG_RT; ++k) zr[k] = lg_lds[roff[k] + o];
#pragma unroll
        for (int m = 0; m < LG_CT; ++m) zc[m] = lg_lds[coff[m] + o];
#pragma unroll
        for (int k = 0; k < LG_RT; ++k)
#pragma unroll
          for (int m = 0; m < LG_CT; ++m) acc[k][m] = fma(zr[k], zc[m], acc[k][m]);
      };
      int w = 0;
      if (UNIT) {
        // LG_UNROLL windows per trip read through the same 12 addresses with immediate offsets; the barriers keep one window's
        // 12 values live at a time, so the registers stay under the 128 that four waves per SIMD allow
        for (; w + LG_UNROLL <= wc; w += LG_UNROLL) {
#pragma unroll
          for (int u = 0; u < LG_UNROLL; ++u) {
            window(w + u);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
#pragma unroll 1
      for (; w < wc; ++w) window(UNIT ? w : w * step);
    }
  }
  if (!worker || n0 + nl >= g.N) return;
  double* out = g.gram + (n0 + nl) * P * (P + H);
#pragma unroll
  for (int k = 0; k < LG_RT; ++k)
#pragma unroll
    for (int m = 0; m < LG_CT; ++m) {
      const int i = rg + a.RG * k, j = cg + a.CG * m;
      if (i < P && j < P + H) out[i * (P + H) + j] = acc[k][m];
    }
}

// gram_pooled[e] = ((gram[0][e] + gram[1][e]) + ...) + gram[N-1][e]: one chain per entry, consecutive threads on consecutive entries
__global__ __launch_bounds__(256) void lin_pool_kernel(const double* gram, double* pooled, int N, int E) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  double sum = 0.0;
  for (int n = 0; n < N; ++n) sum += gram[(int64_t)n * E + e];
  pooled[e] = sum;
}

// ------------------------------------------------------------------ solve: one wave per system, lane = row
// The augmented matrix [G + alpha D | R] sits in LDS with an odd leading dimension; right-looking Cholesky on the lower
// triangle, the forward substitution folded into the elimination (the right-hand sides are further columns), then the
// back substitution.  A block is one wave: __syncthreads() only orders its LDS traffic.
__global__ __launch_bounds__(64) void lin_solve_kernel(TecmLinSolve s) {
  extern __shared__ double ls_lds[];
  const int P = s.P, H = s.H, W = P + H, ld = W | 1;
  const int lane = threadIdx.x;
  const int64_t node = blockIdx.x;
  const double* g = s.gram + node * P * W;
  double* A = ls_lds;                                      // [P][ld]
  double* diag = A + P * ld;                               // [P]: the diagonal of G + alpha D before elimination
  bool finite = true;
  for (int e = lane; e < P * W; e += 64) {
    const int i = e / W, j = e - i * W;
    double v = g[e];
    finite = finite && isfinite(v);
    if (i == j && i > 0) v += s.alpha;
    A[i * ld + j] = v;
    if (i == j) diag[i] = v;
  }
  finite = __syncthreads_and(finite);
  bool ok = true;
  if (finite) {
    for (int k = 0; k < P; ++k) {
      const double p = A[k * ld + k];
      if (!(p > 1e-12 * diag[k])) {                        // the same value in every lane
        ok = false;
        break;
      }
      const double d = sqrt(p);
      __syncthreads();
      if (lane == k) A[k * ld + k] = d;
      if (lane > k && lane < P) A[lane * ld + k] /= d;
      if (lane < H) A[k * ld + P + lane] /= d;              // lanes along the right-hand sides: c_k = R_k / L_kk
      __syncthreads();
      if (lane > k && lane < P) {
        const double lik = A[lane * ld + k];
        for (int j = k + 1; j <= lane; ++j) A[lane * ld + j] -= lik * A[j * ld + k];
        for (int h = 0; h < H; ++h) A[lane * ld + P + h] -= lik * A[k * ld + P + h];
      }
      __syncthreads();
    }
    if (ok)
      for (int k = P - 1; k >= 0; --k) {
        if (lane < H) A[k * ld + P + lane] /= A[k * ld + k];
        __syncthreads();
        if (lane < k) {
          const double lki = A[k * ld + lane];
          for (int h = 0; h < H; ++h) A[lane * ld + P + h] -= lki * A[k * ld + P + h];
        }
        __syncthreads();
      }
  }
  const double nan = __builtin_nan("");
  for (int e = lane; e < P * H; e += 64) {
    const int p = e / H, h = e - p * H;
    double v;
    if (!finite) v = nan;
    else if (!ok) v = p == 0 ? g[h + P] / g[0] : 0.0;      // the intercept-only model: the mean training target
    else v = A[p * ld + P + h];
    s.coef[node * P * H + e] = v;
    if (s.coef_t) s.coef_t[(int64_t)e * s.N + node] = v;
  }
  if (lane == 0) s.status[node] = !finite ? TECM_LIN_NONFINITE : (ok ? 0 : TECM_LIN_DEGENERATE);
}

// ------------------------------------------------------------------ window forecast
// Lanes along nodes (the stride-C channel read of the other baselines).  A thread forecasts WB windows of its node, so a
// coefficient is loaded once for WB fused multiply-adds; LF_GROUPS such groups of windows of the same 64 nodes are stacked
// in one block and share the coefficient tile through the caches.  WB x HB (HB >= H) statically indexed fp64 accumulators.
constexpr int LF_GROUPS = 4;

struct LinForecastArgs {
  TecmLinForecast f;
  int32_t tiles, _pad;
};

template <int HB, int WB>
__global__ __launch_bounds__(64 * LF_GROUPS) void lin_forecast_kernel(LinForecastArgs a) {
  const TecmWindowBaseline& w = a.f.w;
  const int tile = blockIdx.x % a.tiles;
  const int b0 = ((blockIdx.x / a.tiles) * LF_GROUPS + threadIdx.y) * WB;
  const int n = tile * 64 + threadIdx.x;
  if (b0 >= w.B || n >= w.N) return;
  const int H = w.L_out, P = a.f.P;
  const int64_t row = (int64_t)w.N * w.C;
  const float* x[WB];
  bool live[WB];
#pragma unroll
  for (int i = 0; i < WB; ++i) {
    const int b = b0 + i;
    const int64_t start = b < w.B ? w.starts[b] : -1;
    live[i] = start >= 0 && start + w.L_in <= w.T;         // never read outside the series
    if (b < w.B && !live[i]) {
      float* out = w.out + (int64_t)b * w.o_stride_b + (int64_t)n * w.o_stride_n;
      for (int h = 0; h < H; ++h) out[h * w.o_stride_h] = __builtin_nanf("");
    }
    x[i] = w.X + ((live[i] ? start : 0) + w.L_in) * row + (int64_t)n * w.C;      // a dead slot computes on window 0 and stores nothing
  }
  const int64_t ce = a.f.coef_stride_n ? w.N : 1;          // elements between two (p, h) entries
  const double* coef = a.f.coef + (a.f.coef_stride_n ? n : 0);
  double acc[WB][HB];
#pragma unroll
  for (int h = 0; h < HB; ++h) {
    const double c = h < H ? coef[h * ce] : 0.0;
#pragma unroll
    for (int i = 0; i < WB; ++i) acc[i][h] = c;
  }
  for (int p = 1; p < P; ++p) {
    const int64_t at = a.f.chan[p] - a.f.lag[p] * row;
    double z[WB];
#pragma unroll
    for (int i = 0; i < WB; ++i) z[i] = (double)x[i][at];
    const double* c = coef + (int64_t)p * H * ce;
#pragma unroll
    for (int h = 0; h < HB; ++h)
      if (h < H) {
        const double ch = c[h * ce];
#pragma unroll
        for (int i = 0; i < WB; ++i) acc[i][h] = fma(z[i], ch, acc[i][h]);
      }
  }
#pragma unroll
  for (int i = 0; i < WB; ++i)
    if (live[i]) {
      float* out = w.out + (int64_t)(b0 + i) * w.o_stride_b + (int64_t)n * w.o_stride_n;
#pragma unroll
      for (int h = 0; h < HB; ++h)
        if (h < H) out[h * w.o_stride_h] = (float)acc[i][h];
    }
}

template <int HB, int WB>
void lin_forecast_launch(const LinForecastArgs& a, hipStream_t st) {
  const int groups = (a.f.w.B + WB - 1) / WB;
  const unsigned blocks = (unsigned)(a.tiles * ((groups + LF_GROUPS - 1) / LF_GROUPS));
  hipLaunchKernelGGL((lin_forecast_kernel<HB, WB>), dim3(blocks), dim3(64, LF_GROUPS), 0, st, a);
}

// ------------------------------------------------------------------ host side
// Validates the predictor pairs against (C, L_in) and fills the channel slots; returns an error text or nullptr.
const char* lin_pairs(int P, int C, int L_in, const int32_t* chan, const int32_t* lag, int32_t* slot, int32_t* chans, int* nch,
                      int* maxlag) {
  if (P < 1 || P > TECM_LIN_MAX_P) return "P (intercept included) must lie in [1, 64]";
  if (C < 1 || L_in < 1) return "bad shape";
  *nch = 0;
  *maxlag = 0;
  for (int p = 1; p < P; ++p) {
    if (lag[p] < 1 || lag[p] > TECM_LIN_MAX_LAG) return "a look-back must lie in [1, 512]";
    if (lag[p] > L_in) return "a look-back reaches before the input window (lag > L_in)";
    if (chan[p] < 0 || chan[p] >= C) return "a predictor's channel lies outside [0, C)";
    int s = 0;
    while (s < *nch && chans[s] != chan[p]) ++s;
    if (s == *nch) {
      if (*nch == TECM_LIN_MAX_CHANNELS) return "the predictors use more than 8 distinct channels";
      chans[(*nch)++] = chan[p];
    }
    if (slot) slot[p] = s;
    if (lag[p] > *maxlag) *maxlag = lag[p];
  }
  return nullptr;
}

const char* lin_gram_args(const TecmLinGram* g, LinGramArgs* a) {
  if (!g) return "null descriptor";
  const char* bad = lin_pairs(g->P, g->C, g->L_in, g->chan, g->lag, a->slot, a->chans, &a->nch, &a->maxlag);
  if (bad) return bad;
  if (g->H < 1 || g->H > TECM_LIN_MAX_H) return "H must lie in [1, 32]";
  if (g->N < 1 || g->T < 1 || g->Ty < 1) return "bad shape";
  if (g->ys_stride_t < 0 || g->ys_stride_n < 0) return "negative stride";
  if (g->count < 1) return "count < 1: no window to fit";
  if (g->first < 0 || g->step < 1) return "windows must start at first >= 0 and advance by step >= 1";
  if (g->step > 0x3fffffff || g->count > 0x3fffffffffffLL / g->step) return "window progression too long";
  const int64_t last = g->first + (g->count - 1) * g->step;
  if (last + g->L_in > g->T) return "the last window's inputs leave the T rows of X";
  if (last + g->L_in + g->H > g->Ty) return "the last window's targets leave the Ty rows of ys";
  a->g = *g;
  const int halo = a->maxlag + g->H;                       // <= 544
  const int nslots = a->nch + 1;
  // the largest tile of nodes whose LDS share still holds two halos of rows (at most half of a chunk is re-staged); one node fits always
  int tile = LG_MAX_TILE;
  while (tile > 1 && ((LG_LDS_DOUBLES / (tile * nslots + 1)) - 1) < 2 * halo) tile >>= 1;
  const int smax = ((LG_LDS_DOUBLES / (tile * nslots + 1)) - 1) | 1;       // odd: consecutive regions start on different banks
  int64_t chunk = (smax - halo) / g->step + 1;
  if (chunk > g->count) chunk = g->count;
  a->tile = tile;
  a->chunk = (int32_t)chunk;
  a->S = (int32_t)((chunk - 1) * g->step + halo) | 1;
  a->RG = (g->P + LG_RT - 1) / LG_RT;
  a->CG = (g->P + g->H + LG_CT - 1) / LG_CT;
  a->threads = (tile * a->RG * a->CG + 63) / 64 * 64;
  return nullptr;
}

}  // namespace

extern "C" int tecm_lin_gram_supported(const TecmLinGram* g, int32_t* tile_nodes, int32_t* chunk_windows) {
  LinGramArgs a;
  const char* bad = lin_gram_args(g, &a);
  if (bad) {
    tecm_set_error("tecm_lin_gram: %s", bad);
    return 0;
  }
  if (tile_nodes) *tile_nodes = a.tile;
  if (chunk_windows) *chunk_windows = a.chunk;
  return 1;
}

extern "C" int tecm_lin_gram(const TecmLinGram* g, void* stream) {
  LinGramArgs a;
  const char* bad = lin_gram_args(g, &a);
  TECM_REQUIRE(!bad, TECM_E_ARG, "tecm_lin_gram: %s", bad);
  TECM_REQUIRE(g->X && g->ys && g->gram && (!g->pooled || g->gram_pooled), TECM_E_ARG, "tecm_lin_gram: null pointer");
  TECM_REQUIRE(tecm_aligned(g->gram, 8) && tecm_aligned(g->gram_pooled, 8), TECM_E_ALIGN, "tecm_lin_gram: misaligned output");
  const int lds = ((a.tile * (a.nch + 1) + 1) * a.S) * (int)sizeof(double);
  TECM_REQUIRE(lds <= LG_LDS_DOUBLES * (int)sizeof(double) && a.threads <= LG_MAX_THREADS, TECM_E_ARG,
               "tecm_lin_gram: geometry outside the kernel's limits");
  auto kernel = g->step == 1 ? &lin_gram_kernel<true> : &lin_gram_kernel<false>;
  TECM_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 65536) ==
                   hipSuccess,
               TECM_E_LAUNCH, "tecm_lin_gram: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  const unsigned blocks = (unsigned)((g->N + a.tile - 1) / a.tile);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(a.threads), lds, (hipStream_t)stream, a);
  TECM_CHECK_LAUNCH("tecm_lin_gram");
  if (g->pooled) {
    const int E = g->P * (g->P + g->H);
    hipLaunchKernelGGL(lin_pool_kernel, dim3((E + 255) / 256), dim3(256), 0, (hipStream_t)stream, g->gram, g->gram_pooled, g->N, E);
    TECM_CHECK_LAUNCH("tecm_lin_gram (pooled)");
  }
  return TECM_OK;
}

extern "C" int tecm_lin_solve(const TecmLinSolve* s, void* stream) {
  TECM_REQUIRE(s, TECM_E_ARG, "tecm_lin_solve: null descriptor");
  TECM_REQUIRE(s->gram && s->coef && s->status, TECM_E_ARG, "tecm_lin_solve: null pointer");
  TECM_REQUIRE(s->N >= 1 && s->P >= 1 && s->P <= TECM_LIN_MAX_P && s->H >= 1 && s->H <= TECM_LIN_MAX_H, TECM_E_ARG,
               "tecm_lin_solve: needs N >= 1, P in [1, 64] and H in [1, 32]");
  TECM_REQUIRE(s->alpha >= 0.0, TECM_E_ARG, "tecm_lin_solve: alpha must not be negative");
  TECM_REQUIRE(tecm_aligned(s->gram, 8) && tecm_aligned(s->coef, 8) && tecm_aligned(s->coef_t, 8) && tecm_aligned(s->status, 4),
               TECM_E_ALIGN, "tecm_lin_solve: misaligned pointer");
  const int lds = (s->P * ((s->P + s->H) | 1) + s->P) * (int)sizeof(double);           // at most 64 * 97 + 64 doubles = 49 KiB
  if (lds > 32768)
    TECM_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(&lin_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     65536) == hipSuccess,
                 TECM_E_LAUNCH, "tecm_lin_solve: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  hipLaunchKernelGGL(lin_solve_kernel, dim3((unsigned)s->N), dim3(64), lds, (hipStream_t)stream, *s);
  TECM_CHECK_LAUNCH("tecm_lin_solve");
  return TECM_OK;
}

extern "C" int tecm_lin_forecast(const TecmLinForecast* f, void* stream) {
  TECM_REQUIRE(f, TECM_E_ARG, "tecm_lin_forecast: null descriptor");
  const TecmWindowBaseline* w = &f->w;
  TECM_REQUIRE(w->X && w->starts && w->out && f->coef, TECM_E_ARG, "tecm_lin_forecast: null pointer");
  TECM_REQUIRE(w->T > 0 && w->N > 0 && w->C > 0 && w->L_in > 0 && w->L_out > 0 && w->B > 0 && w->L_in <= w->T, TECM_E_ARG,
               "tecm_lin_forecast: bad shape");
  TECM_REQUIRE(w->L_out <= TECM_LIN_MAX_H, TECM_E_ARG, "tecm_lin_forecast: L_out %d exceeds %d", w->L_out, TECM_LIN_MAX_H);
  TECM_REQUIRE(w->L_out == 1 || w->o_stride_h != 0, TECM_E_ARG, "tecm_lin_forecast: needs a non-zero horizon stride");
  TECM_REQUIRE(f->coef_stride_n == 0 || f->coef_stride_n == 1, TECM_E_ARG,
               "tecm_lin_forecast: coef_stride_n must be 1 (node-fastest) or 0 (pooled)");
  TECM_REQUIRE(tecm_aligned(f->coef, 8), TECM_E_ALIGN, "tecm_lin_forecast: coef must be 8-byte aligned");
  int32_t chans[TECM_LIN_MAX_CHANNELS];
  int nch, maxlag;
  const char* bad = lin_pairs(f->P, w->C, w->L_in, f->chan, f->lag, nullptr, chans, &nch, &maxlag);
  TECM_REQUIRE(!bad, TECM_E_ARG, "tecm_lin_forecast: %s", bad);
  if (w->starts_host_check) {
    for (int b = 0; b < w->B; ++b) {
      const int64_t s0 = w->starts_host_check[b];
      TECM_REQUIRE(s0 >= 0 && s0 + w->L_in <= w->T, TECM_E_ARG,
                   "tecm_lin_forecast: window %d starts at %lld, outside [0, T - L_in]", b, (long long)s0);
    }
  }
  LinForecastArgs a;
  a.f = *f;
  a.tiles = (w->N + 63) / 64;
  TECM_REQUIRE((int64_t)a.tiles * w->B <= 0x7fffffffLL, TECM_E_ARG, "tecm_lin_forecast: too many windows for one launch");
  hipStream_t st = (hipStream_t)stream;
  if (w->L_out <= 4) lin_forecast_launch<4, 4>(a, st);
  else if (w->L_out <= 12) lin_forecast_launch<12, 4>(a, st);
  else if (w->L_out <= 24) lin_forecast_launch<24, 2>(a, st);
  else lin_forecast_launch<32, 2>(a, st);
  TECM_CHECK_LAUNCH("tecm_lin_forecast");
  return TECM_OK;
}
