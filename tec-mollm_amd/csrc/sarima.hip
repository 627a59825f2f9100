// SarimaBaseline (the reference's src/models/baselines.py:47-72) on the device: a seasonal ARMA on the differenced series in
// subset form, fitted per node by the two-stage Hannan-Rissanen regression (tecmollm.h (7)), and its forecast for every
// window of a split in one launch.  Every kernel puts lanes along nodes, so one time step is one coalesced row read; all
// arithmetic is fp64.  Per-lane histories (rings of w, e, y; the long AR; Levinson's phi) live in LDS laid out
// [slot][lane], accumulators and coefficients in statically indexed registers: no kernel here uses scratch.
#include "common.h"

namespace {

constexpr int SAR_NODES = 64;                      // one wave per block: a lane only ever touches its own LDS column
constexpr int SAR_K = TECM_SAR_MAX_K;              // 12
constexpr int SAR_M = TECM_SAR_MAX_LONG_AR;        // 64: slots of the w ring of the fit (a power of two)
constexpr int SAR_L = TECM_SAR_MAX_LAG;            // 32: slots of the e ring of the fit (a power of two)
constexpr int SAR_NG = SAR_K * (SAR_K + 1) / 2 + SAR_K + 1;     // 78 of G's upper triangle + 12 of r + wss = 91 partial sums

struct SarLags {
  int32_t lag[SAR_K];      // ar_lags ++ ma_lags
  uint32_t ma_mask;        // bit j: lag[j] addresses e, not w
  int32_t K, Lmax, o;
};

struct SarFitArgs {
  TecmSarFit f;
  SarLags l;
  int64_t n;               // T - o
  int64_t npad;            // 64 * tiles
  int32_t chunks, _pad;
  double* acov_part;       // [chunk][k <= m][npad]
  double* acov_t;          // [k <= m][npad]
  double* phi;             // [i < m][npad]
  double* gram_part;       // [chunk][SAR_NG][npad]
};

// the differenced series at u (t = u + o), from the fp32 series in fp64: (y_t - y_{t-1}) - (y_{t-s} - y_{t-s-1})
__device__ __forceinline__ double sar_w(const float* x, int64_t t, int64_t st, int d, int D, int s) {
  double v = (double)x[t * st];
  if (d) v -= (double)x[(t - 1) * st];
  if (D) {
    double q = (double)x[(t - s) * st];
    if (d) q -= (double)x[(t - s - 1) * st];
    v -= q;
  }
  return v;
}

// ------------------------------------------------------------------ stage 1a: autocovariance partials of one chunk
__global__ __launch_bounds__(SAR_NODES) void sar_autocov_kernel(SarFitArgs a) {
  __shared__ double ring[SAR_M][SAR_NODES];
  const int lane = threadIdx.x;
  const int64_t node = (int64_t)blockIdx.x * SAR_NODES + lane;
  const float* x = a.f.x + (node < a.f.N ? node : 0) * a.f.stride_n;
  const int64_t st = a.f.stride_t;
  const int m = a.f.m, d = a.f.d, D = a.f.D, s = a.f.s, o = a.l.o;
  const int64_t u0 = (int64_t)blockIdx.y * TECM_SAR_CHUNK;
  const int64_t u1 = u0 + TECM_SAR_CHUNK < a.n ? u0 + TECM_SAR_CHUNK : a.n;
  double acc[SAR_M + 1];
#pragma unroll
  for (int k = 0; k <= SAR_M; ++k) acc[k] = 0.0;
  for (int64_t v = u0 > m ? u0 - m : 0; v < u0; ++v) ring[v & (SAR_M - 1)][lane] = sar_w(x, v + o, st, d, D, s);
  for (int64_t u = u0; u < u1; ++u) {
    const double w = sar_w(x, u + o, st, d, D, s);
    const int kmax = u < m ? (int)u : m;
    acc[0] += w * w;
#pragma unroll
    for (int k = 1; k <= SAR_M; ++k)
      if (k <= kmax) acc[k] += w * ring[(u - k) & (SAR_M - 1)][lane];
    ring[u & (SAR_M - 1)][lane] = w;
  }
  double* part = a.acov_part + (int64_t)blockIdx.y * (m + 1) * a.npad + node;
#pragma unroll
  for (int k = 0; k <= SAR_M; ++k)
    if (k <= m) part[(int64_t)k * a.npad] = acc[k];
}

// ------------------------------------------------------------------ stage 1b: join the chunks, Levinson-Durbin
__global__ __launch_bounds__(SAR_NODES) void sar_levinson_kernel(SarFitArgs a) {
  __shared__ double phi[SAR_M][SAR_NODES];
  const int lane = threadIdx.x;
  const int64_t node = (int64_t)blockIdx.x * SAR_NODES + lane;
  const bool live = node < a.f.N;
  const int m = a.f.m;
  double* g = a.acov_t + node;                                   // g[k * npad]: this lane's autocovariances
  for (int k = 0; k <= m; ++k) {
    double sum = 0.0;
    for (int c = 0; c < a.chunks; ++c) sum += a.acov_part[((int64_t)c * (m + 1) + k) * a.npad + node];
    const double v = a.n > 0 ? sum / (double)a.n : 0.0;
    g[(int64_t)k * a.npad] = v;
    if (live) a.f.autocov[node * (m + 1) + k] = v;
  }
  const double g0 = g[0];
  int status = 0;
  if (!isfinite(g0)) status = TECM_SAR_NONFINITE;
  else if (!(g0 > 0.0) || a.n < (int64_t)m + a.l.Lmax + 2 * a.l.K) status = TECM_SAR_DEGENERATE;
  if (status == 0) {
    double var = g0;
    bool ok = true;
    for (int i = 1; i <= m && ok; ++i) {
      double r = g[(int64_t)i * a.npad];
      for (int j = 1; j < i; ++j) r -= phi[j - 1][lane] * g[(int64_t)(i - j) * a.npad];
      const double kap = r / var;
      for (int j = 1; j < i - j; ++j) {                          // phi_j and phi_{i-j} in place
        const double p = phi[j - 1][lane], q = phi[i - j - 1][lane];
        phi[j - 1][lane] = p - kap * q;
        phi[i - j - 1][lane] = q - kap * p;
      }
      if ((i & 1) == 0) {
        const double p = phi[i / 2 - 1][lane];
        phi[i / 2 - 1][lane] = p - kap * p;
      }
      phi[i - 1][lane] = kap;
      var *= 1.0 - kap * kap;
      if (!(var > 0.0)) ok = false;
    }
    if (!ok) status = TECM_SAR_DEGENERATE;
  }
  for (int i = 0; i < m; ++i) a.phi[(int64_t)i * a.npad + node] = status == 0 ? phi[i][lane] : 0.0;
  if (live) a.f.status[node] = status;
}

// ------------------------------------------------------------------ stage 2a: Gram partials of one chunk
// e is a finite filter of w: the chunk rebuilds w from m + Lmax steps and e from Lmax steps before its first row.
__global__ __launch_bounds__(SAR_NODES) void sar_gram_kernel(SarFitArgs a) {
  extern __shared__ double sar_lds[];
  double* wr = sar_lds;                                          // [SAR_M][64]
  double* er = wr + SAR_M * SAR_NODES;                           // [SAR_L][64]
  double* ph = er + SAR_L * SAR_NODES;                           // [SAR_M][64]
  const int lane = threadIdx.x;
  const int64_t node = (int64_t)blockIdx.x * SAR_NODES + lane;
  const float* x = a.f.x + (node < a.f.N ? node : 0) * a.f.stride_n;
  const int64_t st = a.f.stride_t;
  const int m = a.f.m, d = a.f.d, D = a.f.D, s = a.f.s, o = a.l.o, K = a.l.K, Lmax = a.l.Lmax;
  for (int i = 0; i < m; ++i) ph[i * SAR_NODES + lane] = a.phi[(int64_t)i * a.npad + node];
  const int64_t c0 = (int64_t)blockIdx.y * TECM_SAR_CHUNK;
  const int64_t r0 = c0 > m + Lmax ? c0 : m + Lmax;
  const int64_t r1 = c0 + TECM_SAR_CHUNK < a.n ? c0 + TECM_SAR_CHUNK : a.n;
  double G[SAR_K * (SAR_K + 1) / 2], r[SAR_K], wss = 0.0;
#pragma unroll
  for (int i = 0; i < SAR_K * (SAR_K + 1) / 2; ++i) G[i] = 0.0;
#pragma unroll
  for (int i = 0; i < SAR_K; ++i) r[i] = 0.0;
  if (r0 < r1) {
    int64_t v = r0 - Lmax - m;
    for (; v < r0 - Lmax; ++v) wr[(v & (SAR_M - 1)) * SAR_NODES + lane] = sar_w(x, v + o, st, d, D, s);
    for (; v < r1; ++v) {
      const double w = sar_w(x, v + o, st, d, D, s);
      double f = 0.0;
      for (int i = 1; i <= m; ++i) f += ph[(i - 1) * SAR_NODES + lane] * wr[((v - i) & (SAR_M - 1)) * SAR_NODES + lane];
      const double e = w - f;
      if (v >= r0) {
        double z[SAR_K];
#pragma unroll
        for (int j = 0; j < SAR_K; ++j) {
          z[j] = 0.0;
          if (j < K) {
            const int64_t q = v - a.l.lag[j];
            z[j] = (a.l.ma_mask >> j) & 1 ? er[(q & (SAR_L - 1)) * SAR_NODES + lane] : wr[(q & (SAR_M - 1)) * SAR_NODES + lane];
          }
        }
        int idx = 0;
#pragma unroll
        for (int i = 0; i < SAR_K; ++i) {
#pragma unroll
          for (int j = i; j < SAR_K; ++j) G[idx++] += z[i] * z[j];
          r[i] += z[i] * w;
        }
        wss += w * w;
      }
      wr[(v & (SAR_M - 1)) * SAR_NODES + lane] = w;
      er[(v & (SAR_L - 1)) * SAR_NODES + lane] = e;
    }
  }
  double* part = a.gram_part + (int64_t)blockIdx.y * SAR_NG * a.npad + node;
#pragma unroll
  for (int i = 0; i < SAR_K * (SAR_K + 1) / 2; ++i) part[(int64_t)i * a.npad] = G[i];
#pragma unroll
  for (int i = 0; i < SAR_K; ++i) part[(int64_t)(SAR_K * (SAR_K + 1) / 2 + i) * a.npad] = r[i];
  part[(int64_t)(SAR_NG - 1) * a.npad] = wss;
}

// ------------------------------------------------------------------ stage 2b: join the chunks into gram = [G | r] and wss
__global__ __launch_bounds__(SAR_NODES) void sar_gram_join_kernel(SarFitArgs a) {
  const int64_t node = (int64_t)blockIdx.x * SAR_NODES + threadIdx.x;
  if (node >= a.f.N) return;
  const int K = a.l.K;
  double* out = a.f.gram + node * K * (K + 1);
  auto joined = [&](int e) {
    double sum = 0.0;
    for (int c = 0; c < a.chunks; ++c) sum += a.gram_part[((int64_t)c * SAR_NG + e) * a.npad + node];
    return sum;
  };
  int idx = 0;
#pragma unroll 1
  for (int i = 0; i < SAR_K; ++i)
    for (int j = i; j < SAR_K; ++j, ++idx)
      if (j < K) {
        const double v = joined(idx);
        out[i * (K + 1) + j] = v;
        out[j * (K + 1) + i] = v;
      }
  for (int i = 0; i < K; ++i) out[i * (K + 1) + K] = joined(SAR_K * (SAR_K + 1) / 2 + i);
  a.f.wss[node] = joined(SAR_NG - 1);
}

// ------------------------------------------------------------------ solve: one thread per node, K <= 12, unrolled Cholesky
__global__ __launch_bounds__(SAR_NODES) void sar_solve_kernel(TecmSarFit f, int K, int Lmax, int64_t rows) {
  const int64_t node = (int64_t)blockIdx.x * SAR_NODES + threadIdx.x;
  if (node >= f.N) return;
  if (f.use_ma && f.use_ma[node]) return;                        // a second solve touches the chosen nodes only
  const bool drop = f.use_ma != nullptr && f.n_ma > 0;
  const int Ke = drop ? f.n_ar : K;
  int status = f.status[node] & (TECM_SAR_DEGENERATE | TECM_SAR_NONFINITE);
  const double* g = f.gram + node * K * (K + 1);
  const double wss = f.wss[node];
  double A[SAR_K][SAR_K], L[SAR_K][SAR_K], b[SAR_K], c[SAR_K];
#pragma unroll
  for (int i = 0; i < SAR_K; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) A[i][j] = (i < Ke) ? g[i * (K + 1) + j] : (i == j ? 1.0 : 0.0);
    b[i] = i < Ke ? g[i * (K + 1) + K] : 0.0;
  }
  bool ok = true;
#pragma unroll
  for (int k = 0; k < SAR_K; ++k) {
    double p = A[k][k];
#pragma unroll
    for (int j = 0; j < k; ++j) p -= L[k][j] * L[k][j];
    if (k < Ke && !(p > 1e-12 * A[k][k])) ok = false;
    const double dk = sqrt(p);
    L[k][k] = dk;
#pragma unroll
    for (int i = k + 1; i < SAR_K; ++i) {
      double q = A[i][k];
#pragma unroll
      for (int j = 0; j < k; ++j) q -= L[i][j] * L[k][j];
      L[i][k] = q / dk;
    }
  }
#pragma unroll
  for (int i = 0; i < SAR_K; ++i) {
    double q = b[i];
#pragma unroll
    for (int j = 0; j < i; ++j) q -= L[i][j] * c[j];
    c[i] = q / L[i][i];
  }
#pragma unroll
  for (int i = SAR_K - 1; i >= 0; --i) {
    double q = c[i];
#pragma unroll
    for (int j = i + 1; j < SAR_K; ++j) q -= L[j][i] * c[j];
    c[i] = q / L[i][i];
  }
  if (status == 0 && !ok) status = TECM_SAR_DEGENERATE;
  double rss = wss;
#pragma unroll
  for (int i = 0; i < SAR_K; ++i) {
    double q = 0.5 * A[i][i] * c[i];
#pragma unroll
    for (int j = 0; j < i; ++j) q += A[i][j] * c[j];
    rss += 2.0 * c[i] * (q - b[i]);
  }
  double sigma2 = rows > 0 ? rss / (double)rows : 0.0;
  const double nan = __builtin_nan("");
  if (status & TECM_SAR_DEGENERATE) sigma2 = f.autocov[node * (f.m + 1)];
  if (status & TECM_SAR_NONFINITE) sigma2 = nan;
#pragma unroll
  for (int i = 0; i < SAR_K; ++i)
    if (i < K) f.coef[node * K + i] = status & TECM_SAR_NONFINITE ? nan : ((status & TECM_SAR_DEGENERATE) || i >= Ke ? 0.0 : c[i]);
  f.sigma2[node] = sigma2;
  f.status[node] = status | (drop ? TECM_SAR_MA_DROPPED : 0);
}

// ------------------------------------------------------------------ window forecast
// One block per (window, tile of 64 nodes), the tiles of one window on consecutive blocks; one thread per (window, node).
// Rings of w and e (wm + 1 >= Lmax slots) and of y (ym + 1 >= o slots) in LDS; a slot is read before the step that
// overwrites it stores.  Eight loads of the series are issued ahead of the eight steps that consume them.
constexpr int SF_AHEAD = 8;

struct SarForecastArgs {
  TecmSarForecast f;
  SarLags l;
  int32_t tiles, wm, ym, _pad;
};

__global__ __launch_bounds__(SAR_NODES) void sar_forecast_kernel(SarForecastArgs a) {
  extern __shared__ double sar_lds[];
  const TecmWindowBaseline& w = a.f.w;
  const int lane = threadIdx.x;
  const int b = blockIdx.x / a.tiles;
  const int n = (blockIdx.x - b * a.tiles) * SAR_NODES + lane;
  if (n >= w.N) return;
  const int64_t start = w.starts[b];
  float* out = w.out + (int64_t)b * w.o_stride_b + (int64_t)n * w.o_stride_n;
  if (start < 0 || start + w.L_in > w.T) {                       // never read outside the series
    for (int h = 0; h < w.L_out; ++h) out[h * w.o_stride_h] = __builtin_nanf("");
    return;
  }
  const int wm = a.wm, ym = a.ym;
  double* wr = sar_lds + lane;                                   // slot q at wr[(q & wm) * 64]
  double* er = wr + (wm + 1) * SAR_NODES;
  double* yr = er + (wm + 1) * SAR_NODES;
  const int K = a.l.K, Lmax = a.l.Lmax, o = a.l.o, d = a.f.d, D = a.f.D, s = a.f.s;
  double c[SAR_K];
#pragma unroll
  for (int j = 0; j < SAR_K; ++j) c[j] = j < K ? a.f.coef[(int64_t)n * K + j] : 0.0;
  const int64_t row = (int64_t)w.N * w.C;
  const float* x = w.X + start * row + (int64_t)n * w.C + w.channel;

  auto arma = [&](int u) {                                       // sum phi_a w_{u-a} + sum theta_b e_{u-b}
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < SAR_K; ++j)
      if (j < K) {
        const int q = ((u - a.l.lag[j]) & wm) * SAR_NODES;
        acc += c[j] * ((a.l.ma_mask >> j) & 1 ? er[q] : wr[q]);
      }
    return acc;
  };
  auto lagged = [&](int t) {                                     // what the differencing rule adds to w_t to give y_t
    double v = 0.0;
    if (d) v += yr[((t - 1) & ym) * SAR_NODES];
    if (D) {
      double q = yr[((t - s) & ym) * SAR_NODES];
      if (d) q -= yr[((t - s - 1) & ym) * SAR_NODES];
      v += q;
    }
    return v;
  };
  auto step = [&](int t, double y) {
    if (t >= o) {
      const int u = t - o;
      const double wu = y - lagged(t);
      const double e = u >= Lmax ? wu - arma(u) : 0.0;
      wr[(u & wm) * SAR_NODES] = wu;
      er[(u & wm) * SAR_NODES] = e;
    }
    yr[(t & ym) * SAR_NODES] = y;
  };
  int t = 0;
  for (; t + SF_AHEAD <= w.L_in; t += SF_AHEAD) {
    float v[SF_AHEAD];
#pragma unroll
    for (int j = 0; j < SF_AHEAD; ++j) v[j] = x[(int64_t)(t + j) * row];
#pragma unroll
    for (int j = 0; j < SF_AHEAD; ++j) step(t + j, (double)v[j]);
  }
  for (; t < w.L_in; ++t) step(t, (double)x[(int64_t)t * row]);
  for (int h = 0; h < w.L_out; ++h) {
    const int tt = w.L_in + h, u = tt - o;
    const double wh = arma(u);
    const double yh = wh + lagged(tt);
    wr[(u & wm) * SAR_NODES] = wh;
    er[(u & wm) * SAR_NODES] = 0.0;
    yr[(tt & ym) * SAR_NODES] = yh;
    out[h * w.o_stride_h] = (float)yh;
  }
}

// ------------------------------------------------------------------ host side
int pow2_at_least(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

// Validates the model's shape and fills `l`; returns an error text or nullptr.
const char* sar_lags(int d, int D, int s, int n_ar, const int32_t* ar, int n_ma, const int32_t* ma, SarLags* l) {
  if ((d != 0 && d != 1) || (D != 0 && D != 1)) return "d and D must be 0 or 1";
  if (D && s < 1) return "D = 1 needs a period s >= 1";
  if (n_ar < 0 || n_ma < 0 || n_ar + n_ma < 1 || n_ar + n_ma > TECM_SAR_MAX_K) return "1 <= n_ar + n_ma <= 12";
  const int64_t o = (int64_t)d + (D ? (int64_t)s : 0);
  if (o > TECM_SAR_MAX_OFFSET) return "the differencing offset d + s*D must not exceed 64";
  l->K = n_ar + n_ma;
  l->o = (int)o;
  l->Lmax = 0;
  l->ma_mask = 0;
  for (int j = 0; j < SAR_K; ++j) l->lag[j] = 0;
  for (int j = 0; j < l->K; ++j) {
    const bool is_ma = j >= n_ar;
    const int lag = is_ma ? ma[j - n_ar] : ar[j];
    const int prev = (j == 0 || j == n_ar) ? 0 : l->lag[j - 1];
    if (lag <= prev || lag > TECM_SAR_MAX_LAG) return "lags must be ascending, positive and at most 32";
    l->lag[j] = lag;
    if (is_ma) l->ma_mask |= 1u << j;
    if (lag > l->Lmax) l->Lmax = lag;
  }
  return nullptr;
}

const char* sar_fit_args(const TecmSarFit* f, SarFitArgs* a) {
  if (!f) return "null descriptor";
  const char* bad = sar_lags(f->d, f->D, f->s, f->n_ar, f->ar_lags, f->n_ma, f->ma_lags, &a->l);
  if (bad) return bad;
  if (f->T <= 0 || f->N <= 0) return "bad shape";
  if (f->m < a->l.Lmax || f->m > TECM_SAR_MAX_LONG_AR) return "the long AR order m must lie in [Lmax, 64]";
  a->f = *f;
  a->n = f->T - a->l.o;
  a->npad = (int64_t)((f->N + SAR_NODES - 1) / SAR_NODES) * SAR_NODES;
  const int64_t chunks = a->n > 0 ? (a->n + TECM_SAR_CHUNK - 1) / TECM_SAR_CHUNK : 1;
  if (chunks > 65535) return "series too long for one launch (65535 chunks)";
  a->chunks = (int32_t)chunks;
  a->acov_part = f->ws;
  a->acov_t = a->acov_part + chunks * (f->m + 1) * a->npad;
  a->phi = a->acov_t + (int64_t)(f->m + 1) * a->npad;
  a->gram_part = a->phi + (int64_t)f->m * a->npad;
  return nullptr;
}

int64_t sar_ws_doubles(const SarFitArgs& a) {
  return a.npad * ((int64_t)a.chunks * (a.f.m + 1) + (a.f.m + 1) + a.f.m + (int64_t)a.chunks * SAR_NG);
}

}  // namespace

extern "C" int64_t tecm_sar_fit_ws_bytes(const TecmSarFit* f) {
  SarFitArgs a;
  const char* bad = sar_fit_args(f, &a);
  if (bad) {
    tecm_set_error("tecm_sar_fit_ws_bytes: %s", bad);
    return -1;
  }
  return sar_ws_doubles(a) * (int64_t)sizeof(double);
}

extern "C" int tecm_sar_solve(const TecmSarFit* f, void* stream) {
  SarFitArgs a;
  const char* bad = sar_fit_args(f, &a);
  TECM_REQUIRE(!bad, TECM_E_ARG, "tecm_sar_solve: %s", bad);
  TECM_REQUIRE(f->autocov && f->gram && f->wss && f->coef && f->sigma2 && f->status, TECM_E_ARG, "tecm_sar_solve: null pointer");
  TECM_REQUIRE(tecm_aligned(f->autocov, 8) && tecm_aligned(f->gram, 8) && tecm_aligned(f->wss, 8) && tecm_aligned(f->coef, 8) &&
                   tecm_aligned(f->sigma2, 8) && tecm_aligned(f->status, 4),
               TECM_E_ALIGN, "tecm_sar_solve: misaligned output");
  const int64_t rows = a.n - f->m - a.l.Lmax;
  hipLaunchKernelGGL(sar_solve_kernel, dim3((unsigned)(a.npad / SAR_NODES)), dim3(SAR_NODES), 0, (hipStream_t)stream, *f, a.l.K,
                     a.l.Lmax, rows);
  TECM_CHECK_LAUNCH("tecm_sar_solve");
  return TECM_OK;
}

extern "C" int tecm_sar_fit(const TecmSarFit* f, void* stream) {
  SarFitArgs a;
  const char* bad = sar_fit_args(f, &a);
  TECM_REQUIRE(!bad, TECM_E_ARG, "tecm_sar_fit: %s", bad);
  TECM_REQUIRE(f->x && f->ws && f->autocov && f->gram && f->wss && f->coef && f->sigma2 && f->status, TECM_E_ARG,
               "tecm_sar_fit: null pointer");
  TECM_REQUIRE(f->stride_t >= 0 && f->stride_n >= 0, TECM_E_ARG, "tecm_sar_fit: negative stride");
  TECM_REQUIRE(tecm_aligned(f->ws, 8), TECM_E_ALIGN, "tecm_sar_fit: ws must be 8-byte aligned");
  static const int gram_lds = (2 * SAR_M + SAR_L) * SAR_NODES * (int)sizeof(double);
  TECM_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(&sar_gram_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   gram_lds) == hipSuccess,
               TECM_E_LAUNCH, "tecm_sar_fit: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  hipStream_t st = (hipStream_t)stream;
  const unsigned tiles = (unsigned)(a.npad / SAR_NODES);
  TecmSarFit first = *f;
  first.use_ma = nullptr;                                        // the fit solves every node with its MA part
  a.f = first;
  hipLaunchKernelGGL(sar_autocov_kernel, dim3(tiles, a.chunks), dim3(SAR_NODES), 0, st, a);
  TECM_CHECK_LAUNCH("tecm_sar_fit (autocovariances)");
  hipLaunchKernelGGL(sar_levinson_kernel, dim3(tiles), dim3(SAR_NODES), 0, st, a);
  TECM_CHECK_LAUNCH("tecm_sar_fit (Levinson)");
  hipLaunchKernelGGL(sar_gram_kernel, dim3(tiles, a.chunks), dim3(SAR_NODES), gram_lds, st, a);
  TECM_CHECK_LAUNCH("tecm_sar_fit (Gram sums)");
  hipLaunchKernelGGL(sar_gram_join_kernel, dim3(tiles), dim3(SAR_NODES), 0, st, a);
  TECM_CHECK_LAUNCH("tecm_sar_fit (join)");
  return tecm_sar_solve(&first, stream);
}

extern "C" int tecm_sar_forecast(const TecmSarForecast* f, void* stream) {
  TECM_REQUIRE(f, TECM_E_ARG, "tecm_sar_forecast: null descriptor");
  const TecmWindowBaseline* w = &f->w;
  TECM_REQUIRE(w->X && w->starts && w->out && f->coef, TECM_E_ARG, "tecm_sar_forecast: null pointer");
  TECM_REQUIRE(w->T > 0 && w->N > 0 && w->C > 0 && w->L_in > 0 && w->L_out > 0 && w->B > 0 && w->L_in <= w->T, TECM_E_ARG,
               "tecm_sar_forecast: bad shape");
  TECM_REQUIRE(w->channel >= 0 && w->channel < w->C, TECM_E_ARG, "tecm_sar_forecast: channel %d outside [0, %d)", w->channel,
               w->C);
  TECM_REQUIRE(w->L_out == 1 || w->o_stride_h != 0, TECM_E_ARG, "tecm_sar_forecast: needs a non-zero horizon stride");
  TECM_REQUIRE(tecm_aligned(f->coef, 8), TECM_E_ALIGN, "tecm_sar_forecast: coef must be 8-byte aligned");
  SarForecastArgs a;
  const char* bad = sar_lags(f->d, f->D, f->s, f->n_ar, f->ar_lags, f->n_ma, f->ma_lags, &a.l);
  TECM_REQUIRE(!bad, TECM_E_ARG, "tecm_sar_forecast: %s", bad);
  TECM_REQUIRE(w->L_in >= a.l.o + a.l.Lmax + 1, TECM_E_ARG, "tecm_sar_forecast: L_in %d is shorter than o + Lmax + 1 = %d", w->L_in,
               a.l.o + a.l.Lmax + 1);
  TECM_REQUIRE((int64_t)w->L_in + w->L_out <= 0x3fffffffLL, TECM_E_ARG, "tecm_sar_forecast: window too long");
  if (w->starts_host_check) {
    for (int b = 0; b < w->B; ++b) {
      const int64_t s0 = w->starts_host_check[b];
      TECM_REQUIRE(s0 >= 0 && s0 + w->L_in <= w->T, TECM_E_ARG,
                   "tecm_sar_forecast: window %d starts at %lld, outside [0, T - L_in]", b, (long long)s0);
    }
  }
  a.f = *f;
  a.tiles = (w->N + SAR_NODES - 1) / SAR_NODES;
  TECM_REQUIRE((int64_t)a.tiles * w->B <= 0x7fffffffLL, TECM_E_ARG, "tecm_sar_forecast: too many windows for one launch");
  a.wm = pow2_at_least(a.l.Lmax) - 1;
  a.ym = pow2_at_least(a.l.o > 1 ? a.l.o : 1) - 1;
  const int lds = (2 * (a.wm + 1) + (a.ym + 1)) * SAR_NODES * (int)sizeof(double);         // at most (64 + 64) * 512 = 64 KiB
  if (lds > 32768)
    TECM_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(&sar_forecast_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     65536) == hipSuccess,
                 TECM_E_LAUNCH, "tecm_sar_forecast: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  hipLaunchKernelGGL(sar_forecast_kernel, dim3((unsigned)(a.tiles * w->B)), dim3(SAR_NODES), lds, (hipStream_t)stream, a);
  TECM_CHECK_LAUNCH("tecm_sar_forecast");
  return TECM_OK;
}
