// The raw-data stage (scripts/preprocess.py over src/features/feature_engineering.py): the scaler fits as weighted fp64
// moments of the raw series, and the feature / target tensors of a split from the raw series and the fitted scalers.
// All kernels stream: tecm_moments reads its input twice, tecm_features_build writes each output once.
#include "common.h"

namespace {

// ------------------------------------------------------------------ fp64 moments
// A thread's running sum: seven accumulators, level i carrying into level i + 1 every 64 carries, so that no accumulator
// takes more than 63 dependent additions (the last: 2^40 / 2^36 = 16) however many entries the thread is given.
struct Cascade {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0, a6 = 0.0;
  uint64_t k = 0;
  __device__ __forceinline__ void add(double v) {
    a0 += v;
    if ((++k & 63u) == 0) carry();
  }
  __device__ __forceinline__ void carry() {
    a1 += a0; a0 = 0.0;
    if (k & 0xfffull) return;
    a2 += a1; a1 = 0.0;
    if (k & 0x3ffffull) return;
    a3 += a2; a2 = 0.0;
    if (k & 0xffffffull) return;
    a4 += a3; a3 = 0.0;
    if (k & 0x3fffffffull) return;
    a5 += a4; a4 = 0.0;
    if (k & 0xfffffffffull) return;
    a6 += a5; a5 = 0.0;
  }
  __device__ __forceinline__ double total() const { return (((((a6 + a5) + a4) + a3) + a2) + a1) + a0; }
};

__device__ __forceinline__ double block_tree_f64(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ long long block_tree_i64(long long v, long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// the number of targets of construct_target_tensor_Y (feature_engineering.py:63-65) that hold row r
__device__ __forceinline__ int row_weight(int64_t r, int64_t rows, int taps) {
  if (taps == 0) return 1;
  const int64_t hi = r - 1 < taps - 1 ? r - 1 : taps - 1;
  const int64_t lo = r - rows + taps > 0 ? r - rows + taps : 0;
  return hi >= lo ? (int)(hi - lo + 1) : 0;
}

struct Partial {
  double sum;
  long long count;
};

// PASS 0: sum w x and the count.  PASS 1: sum w (x - mean)^2 with the mean of pass 0 read from the device.
template <typename T, int PASS>
__device__ __forceinline__ void moments_add(Cascade& acc, long long& cnt, T raw, int w, double mean) {
  const double x = (double)raw;
  const bool ok = x == x && w != 0;                                  // NaN entries and rows no target holds add nothing
  if (PASS == 0) {
    acc.add(ok ? (double)w * x : 0.0);
    cnt += ok ? w : 0;
  } else {
    const double d = x - mean;
    acc.add(ok ? (double)w * (d * d) : 0.0);
  }
}

// pooled: blockIdx.x walks 256-column chunks, blockIdx.y rows; a row of a chunk is one coalesced read
template <typename T, int PASS>
__global__ __launch_bounds__(256) void moments_pool_kernel(TecmMoments m, Partial* __restrict__ part) {
  __shared__ double red[4];
  __shared__ long long redi[4];
  const T* src = static_cast<const T*>(m.src);
  const double mean = PASS == 1 ? m.mean[0] : 0.0;
  Cascade acc;
  long long cnt = 0;
  const int64_t gy = gridDim.y;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < m.cols; c += (int64_t)gridDim.x * 256) {
    const T* col = src + c;
    int64_t r = blockIdx.y;
    for (; r + 3 * gy < m.rows; r += 4 * gy) {                       // four rows' loads in flight, added in row order
      const T v0 = col[r * m.ld], v1 = col[(r + gy) * m.ld], v2 = col[(r + 2 * gy) * m.ld], v3 = col[(r + 3 * gy) * m.ld];
      moments_add<T, PASS>(acc, cnt, v0, row_weight(r, m.rows, m.taps), mean);
      moments_add<T, PASS>(acc, cnt, v1, row_weight(r + gy, m.rows, m.taps), mean);
      moments_add<T, PASS>(acc, cnt, v2, row_weight(r + 2 * gy, m.rows, m.taps), mean);
      moments_add<T, PASS>(acc, cnt, v3, row_weight(r + 3 * gy, m.rows, m.taps), mean);
    }
    for (; r < m.rows; r += gy) moments_add<T, PASS>(acc, cnt, col[r * m.ld], row_weight(r, m.rows, m.taps), mean);
  }
  const double s = block_tree_f64(acc.total(), red);
  const long long n = PASS == 0 ? block_tree_i64(cnt, redi) : 0;
  if (threadIdx.x == 0) {
    Partial& p = part[blockIdx.y * gridDim.x + blockIdx.x];
    p.sum = s;
    if (PASS == 0) p.count = n;
  }
}

// per column: blockIdx.y is the column, lanes run along the rows
template <typename T, int PASS>
__global__ __launch_bounds__(256) void moments_col_kernel(TecmMoments m, Partial* __restrict__ part) {
  __shared__ double red[4];
  __shared__ long long redi[4];
  const int64_t c = blockIdx.y;
  const T* src = static_cast<const T*>(m.src) + c;
  const double mean = PASS == 1 ? m.mean[c] : 0.0;
  Cascade acc;
  long long cnt = 0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < m.rows; r += (int64_t)gridDim.x * 256)
    moments_add<T, PASS>(acc, cnt, src[r * m.ld], row_weight(r, m.rows, m.taps), mean);
  const double s = block_tree_f64(acc.total(), red);
  const long long n = PASS == 0 ? block_tree_i64(cnt, redi) : 0;
  if (threadIdx.x == 0) {
    Partial& p = part[c * gridDim.x + blockIdx.x];
    p.sum = s;
    if (PASS == 0) p.count = n;
  }
}

// one block per statistic joins its partials: thread t adds partials t, t + 256, ... (at most 8) in ascending order
template <int PASS>
__global__ __launch_bounds__(256) void moments_join_kernel(TecmMoments m, const Partial* __restrict__ part, int per_stat) {
  __shared__ double red[4];
  __shared__ long long redi[4];
  const Partial* p = part + (int64_t)blockIdx.x * per_stat;
  double s = 0.0;
  long long n = 0;
  for (int i = threadIdx.x; i < per_stat; i += 256) {
    s += p[i].sum;
    if (PASS == 0) n += p[i].count;
  }
  s = block_tree_f64(s, red);
  if (PASS == 0) n = block_tree_i64(n, redi);
  if (threadIdx.x == 0) {
    if (PASS == 0) {
      m.count[blockIdx.x] = n;
      m.mean[blockIdx.x] = s / (double)n;                            // 0 / 0: NaN for a statistic with no entry
    } else {
      m.var[blockIdx.x] = s / (double)m.count[blockIdx.x];
    }
  }
}

struct MomentsGrid {
  int gx, gy, per_stat;
  int64_t stats;
};

bool moments_grid(const TecmMoments* m, MomentsGrid* g) {
  if (!m || m->rows <= 0 || m->cols <= 0 || m->ld < m->cols) return false;
  if (m->rows > ((int64_t)1 << 40) / m->cols) return false;
  if (m->pool) {
    const int64_t chunks = (m->cols + 255) / 256;
    g->gx = (int)(chunks < TECM_MOMENTS_MAX_BLOCKS ? chunks : TECM_MOMENTS_MAX_BLOCKS);
    const int64_t room = TECM_MOMENTS_MAX_BLOCKS / g->gx;
    g->gy = (int)(m->rows < room ? m->rows : room);
    g->per_stat = g->gx * g->gy;
    g->stats = 1;
  } else {
    if (m->cols > 65535) return false;
    const int64_t want = (m->rows + 256 * 8 - 1) / (256 * 8);
    g->gx = (int)(want < 256 ? want : 256);
    g->gy = (int)m->cols;
    g->per_stat = g->gx;
    g->stats = m->cols;
  }
  return true;
}

template <typename T>
int moments_launch(const TecmMoments* m, const MomentsGrid& g, hipStream_t st) {
  Partial* part = static_cast<Partial*>(m->ws);
  const dim3 grid(g.gx, g.gy);
  if (m->pool) hipLaunchKernelGGL((moments_pool_kernel<T, 0>), grid, dim3(256), 0, st, *m, part);
  else hipLaunchKernelGGL((moments_col_kernel<T, 0>), grid, dim3(256), 0, st, *m, part);
  TECM_CHECK_LAUNCH("tecm_moments/sum");
  hipLaunchKernelGGL(moments_join_kernel<0>, dim3((int)g.stats), dim3(256), 0, st, *m, part, g.per_stat);
  TECM_CHECK_LAUNCH("tecm_moments/mean");
  if (m->pool) hipLaunchKernelGGL((moments_pool_kernel<T, 1>), grid, dim3(256), 0, st, *m, part);
  else hipLaunchKernelGGL((moments_col_kernel<T, 1>), grid, dim3(256), 0, st, *m, part);
  TECM_CHECK_LAUNCH("tecm_moments/squares");
  hipLaunchKernelGGL(moments_join_kernel<1>, dim3((int)g.stats), dim3(256), 0, st, *m, part, g.per_stat);
  TECM_CHECK_LAUNCH("tecm_moments/var");
  return TECM_OK;
}

// ------------------------------------------------------------------ feature and target tensors
struct FeatureScalers {
  double mean[1 + TECM_FEATURES_MAX_CI], scale[1 + TECM_FEATURES_MAX_CI];
};

// one fp64 subtraction, one IEEE fp64 division, one RNE conversion: StandardScaler.transform then .float()
__device__ __forceinline__ float standardise(double v, double mean, double scale) { return (float)((v - mean) / scale); }

// The floats [first, last) of `out` belong to the caller's row.  Threads own the absolutely aligned quads that overlap
// them: a whole quad is one float4 store (vec), a quad cut by the row boundary -- its other floats belong to the
// neighbouring row's block -- and every quad of an unaligned `out` scalar stores.  f(j) is the value of float first + j,
// f4(j) the values of the floats first + j .. first + j + 3 (one division to place the first, steps for the rest).
template <class F, class F4>
__device__ __forceinline__ void fill_row(float* __restrict__ out, int64_t first, int64_t last, int vec, F f, F4 f4) {
  const int64_t q_lo = first >> 2, q_hi = (last + 3) >> 2;
  for (int64_t q = q_lo + (int64_t)blockIdx.x * 256 + threadIdx.x; q < q_hi; q += (int64_t)gridDim.x * 256) {
    const int64_t o = q << 2;
    if (vec && o >= first && o + 4 <= last) {
      *reinterpret_cast<float4*>(out + o) = f4(o - first);
    } else {
      const int64_t lo = o > first ? o : first, hi = o + 4 < last ? o + 4 : last;
      for (int64_t e = lo; e < hi; ++e) out[e] = f(e - first);
    }
  }
}

// X[t, n, c]: channel 0 from tec[t, n]; channels 1.. are the row's Ci index values, standardised once per block into LDS
template <typename T>
__global__ __launch_bounds__(256) void features_x_kernel(TecmFeaturesBuild f, FeatureScalers s, int vec) {
  __shared__ float idx_row[TECM_FEATURES_MAX_CI];
  const unsigned C = 1 + f.Ci;
  const int64_t len = (int64_t)f.N * C;
  for (int64_t t = blockIdx.y; t < f.x_rows; t += gridDim.y) {
    __syncthreads();
    if ((int)threadIdx.x < f.Ci) {
      const int64_t at = t * f.Ci + threadIdx.x;
      const double v = f.idx_f64 ? static_cast<const double*>(f.idx)[at] : (double)static_cast<const float*>(f.idx)[at];
      idx_row[threadIdx.x] = standardise(v, s.mean[1 + threadIdx.x], s.scale[1 + threadIdx.x]);
    }
    __syncthreads();
    const T* tec = static_cast<const T*>(f.tec) + t * f.N;
    const auto value = [&](unsigned n, unsigned c) {
      return c == 0 ? standardise((double)tec[n], s.mean[0], s.scale[0]) : idx_row[c - 1];
    };
    fill_row(f.X, t * len, (t + 1) * len, vec,
             [&](int64_t j) {
               const unsigned n = (unsigned)j / C;
               return value(n, (unsigned)j - n * C);
             },
             [&](int64_t j) {
               unsigned n = (unsigned)j / C, c = (unsigned)j - n * C;
               float4 v;
               v.x = value(n, c); if (++c == C) { c = 0; ++n; }
               v.y = value(n, c); if (++c == C) { c = 0; ++n; }
               v.z = value(n, c); if (++c == C) { c = 0; ++n; }
               v.w = value(n, c);
               return v;
             });
  }
}

// Ys[t, n]: elementwise over the whole series
template <typename T>
__global__ __launch_bounds__(256) void features_ys_kernel(TecmFeaturesBuild f, int vec) {
  const T* tec = static_cast<const T*>(f.tec);
  const int64_t total = f.rows * f.N;
  const int64_t quads = vec ? total >> 2 : 0;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
    const T* p = static_cast<const T*>(__builtin_assume_aligned(tec + (q << 2), 4 * sizeof(T)));
    float4 v;
    v.x = standardise((double)p[0], f.ymean, f.yscale);
    v.y = standardise((double)p[1], f.ymean, f.yscale);
    v.z = standardise((double)p[2], f.ymean, f.yscale);
    v.w = standardise((double)p[3], f.ymean, f.yscale);
    reinterpret_cast<float4*>(f.Ys)[q] = v;
  }
  for (int64_t e = (quads << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256)
    f.Ys[e] = standardise((double)tec[e], f.ymean, f.yscale);
}

// Y[t, n, h] = the Ys value of tec[t + 1 + h, n]
template <typename T>
__global__ __launch_bounds__(256) void features_y_kernel(TecmFeaturesBuild f, int vec) {
  const unsigned H = f.H;
  const int64_t len = (int64_t)f.N * H;
  for (int64_t t = blockIdx.y; t < f.rows - f.H; t += gridDim.y) {
    const T* tec = static_cast<const T*>(f.tec) + (t + 1) * f.N;
    const auto value = [&](unsigned n, unsigned h) { return standardise((double)tec[(int64_t)h * f.N + n], f.ymean, f.yscale); };
    fill_row(f.Y, t * len, (t + 1) * len, vec,
             [&](int64_t j) {
               const unsigned n = (unsigned)j / H;
               return value(n, (unsigned)j - n * H);
             },
             [&](int64_t j) {
               unsigned n = (unsigned)j / H, h = (unsigned)j - n * H;
               float4 v;
               v.x = value(n, h); if (++h == H) { h = 0; ++n; }
               v.y = value(n, h); if (++h == H) { h = 0; ++n; }
               v.z = value(n, h); if (++h == H) { h = 0; ++n; }
               v.w = value(n, h);
               return v;
             });
  }
}

int row_blocks(int64_t len) {
  const int64_t want = ((len >> 2) + 2 + 511) / 512;                 // two quads a thread
  return (int)(want < 1 ? 1 : (want < 64 ? want : 64));
}

template <typename T>
int features_launch(const TecmFeaturesBuild* f, const FeatureScalers& s, hipStream_t st) {
  if (f->X && f->x_rows > 0) {
    const int64_t len = (int64_t)f->N * (1 + f->Ci);
    const int gy = (int)(f->x_rows < 65535 ? f->x_rows : 65535);
    hipLaunchKernelGGL(features_x_kernel<T>, dim3(row_blocks(len), gy), dim3(256), 0, st, *f, s, (int)tecm_aligned(f->X, 16));
    TECM_CHECK_LAUNCH("tecm_features_build/X");
  }
  if (f->Ys) {
    // the vector path reads four source values a thread: needs the source aligned to four of them as well
    const int vec = tecm_aligned(f->Ys, 16) && tecm_aligned(f->tec, 4 * sizeof(T));
    const int64_t want = (f->rows * f->N / 4 + 255) / 256;
    const int gx = (int)(want < 1 ? 1 : (want < 8192 ? want : 8192));
    hipLaunchKernelGGL(features_ys_kernel<T>, dim3(gx), dim3(256), 0, st, *f, vec);
    TECM_CHECK_LAUNCH("tecm_features_build/Ys");
  }
  if (f->Y) {
    const int64_t len = (int64_t)f->N * f->H, yr = f->rows - f->H;
    const int gy = (int)(yr < 65535 ? yr : 65535);
    hipLaunchKernelGGL(features_y_kernel<T>, dim3(row_blocks(len), gy), dim3(256), 0, st, *f, (int)tecm_aligned(f->Y, 16));
    TECM_CHECK_LAUNCH("tecm_features_build/Y");
  }
  return TECM_OK;
}

}  // namespace

extern "C" int64_t tecm_moments_ws_bytes(const TecmMoments* m) {
  MomentsGrid g;
  if (!moments_grid(m, &g)) return -1;
  return g.stats * g.per_stat * (int64_t)sizeof(Partial);
}

extern "C" int tecm_moments(const TecmMoments* m, void* stream) {
  TECM_REQUIRE(m, TECM_E_ARG, "tecm_moments: null descriptor");
  TECM_REQUIRE(m->src && m->count && m->mean && m->var && m->ws, TECM_E_ARG, "tecm_moments: null pointer");
  TECM_REQUIRE(m->src_f64 == 0 || m->src_f64 == 1, TECM_E_ARG, "tecm_moments: src_f64 must be 0 (float32) or 1 (float64)");
  TECM_REQUIRE(m->pool == 0 || m->pool == 1, TECM_E_ARG, "tecm_moments: pool must be 0 or 1");
  MomentsGrid g;
  TECM_REQUIRE(moments_grid(m, &g), TECM_E_ARG,
               "tecm_moments: bad shape (0 < cols <= ld, rows * cols < 2^40, at most 65535 columns without pool)");
  TECM_REQUIRE(m->taps >= 0 && m->taps < m->rows, TECM_E_ARG, "tecm_moments: taps must lie in [0, rows)");
  TECM_REQUIRE(tecm_aligned(m->src, m->src_f64 ? 8 : 4) && tecm_aligned(m->count, 8) && tecm_aligned(m->mean, 8) &&
                   tecm_aligned(m->var, 8) && tecm_aligned(m->ws, 8),
               TECM_E_ALIGN, "tecm_moments: src must be aligned to its element, count / mean / var / ws to 8 bytes");
  hipStream_t st = (hipStream_t)stream;
  return m->src_f64 ? moments_launch<double>(m, g, st) : moments_launch<float>(m, g, st);
}

extern "C" int tecm_features_build(const TecmFeaturesBuild* f, void* stream) {
  TECM_REQUIRE(f, TECM_E_ARG, "tecm_features_build: null descriptor");
  TECM_REQUIRE(f->tec && (f->X || f->Ys || f->Y), TECM_E_ARG, "tecm_features_build: null pointer (tec and one output)");
  TECM_REQUIRE((f->tec_f64 == 0 || f->tec_f64 == 1) && (f->idx_f64 == 0 || f->idx_f64 == 1), TECM_E_ARG,
               "tecm_features_build: tec_f64 and idx_f64 must be 0 (float32) or 1 (float64)");
  TECM_REQUIRE(f->rows > 0 && f->N > 0 && f->x_rows >= 0 && f->x_rows <= f->rows, TECM_E_ARG,
               "tecm_features_build: bad shape (rows, N > 0 and 0 <= x_rows <= rows)");
  TECM_REQUIRE(f->Ci >= 0 && f->Ci <= TECM_FEATURES_MAX_CI, TECM_E_ARG, "tecm_features_build: Ci outside [0, %d]",
               TECM_FEATURES_MAX_CI);
  TECM_REQUIRE((int64_t)f->N * (1 + TECM_FEATURES_MAX_CI) < ((int64_t)1 << 31), TECM_E_ARG, "tecm_features_build: N too large");
  FeatureScalers s = {};
  if (f->X) {
    TECM_REQUIRE(f->mean && f->scale && (f->Ci == 0 || f->idx), TECM_E_ARG,
                 "tecm_features_build: X needs mean, scale and (with Ci > 0) idx");
    for (int c = 0; c <= f->Ci; ++c) {
      TECM_REQUIRE(f->scale[c] != 0.0, TECM_E_ARG, "tecm_features_build: scale[%d] must be non-zero", c);
      s.mean[c] = f->mean[c];
      s.scale[c] = f->scale[c];
    }
  }
  TECM_REQUIRE(!(f->Ys || f->Y) || f->yscale != 0.0, TECM_E_ARG, "tecm_features_build: yscale must be non-zero");
  TECM_REQUIRE(!f->Y || (f->H > 0 && f->H < f->rows && (int64_t)f->N * f->H < ((int64_t)1 << 31)), TECM_E_ARG,
               "tecm_features_build: Y needs 0 < H < rows");
  TECM_REQUIRE(tecm_aligned(f->tec, f->tec_f64 ? 8 : 4) && tecm_aligned(f->idx, f->idx_f64 ? 8 : 4) && tecm_aligned(f->X, 4) &&
                   tecm_aligned(f->Ys, 4) && tecm_aligned(f->Y, 4),
               TECM_E_ALIGN, "tecm_features_build: every pointer must be aligned to its element");
  hipStream_t st = (hipStream_t)stream;
  return f->tec_f64 ? features_launch<double>(f, s, st) : features_launch<float>(f, s, st);
}
