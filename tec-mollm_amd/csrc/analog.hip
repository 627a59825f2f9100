// AnalogBaseline (tecmollm.h (10)) on the device: for every (query window, node) the K stretches of the node's archive that
// lie nearest to the query's last m input steps (analog_search_kernel, the hot path) and the forecast made of what followed
// them (analog_forecast_kernel).  The table of distances, S x N x Ta floats, is never stored: the selection runs inside the sweep.
//
// Search geometry.  A block of four waves owns one node and a tile of AN_QT queries and walks the node's archive, one
// contiguous run of the node-major (N, Ta) array, in chunks of AN_CHUNK candidates staged in LDS with a halo of m - 1 rows.
// The tile's query segments sit in LDS as [query][step] and are read by broadcast, four steps per ds_read_b128.  Lane i takes the
// candidates c0 + i, c0 + 256 + i and c0 + 512 + i, so the reads of A[c + l] of one instruction touch consecutive LDS words,
// and keeps AN_QT x AN_CT running sums: per four steps 12 + 4 LDS reads feed 96 subtract / multiply-add pairs, which leaves
// the sweep bound by the vector ALU.
//
// Selection.  Every wave keeps, per query of the tile, its K best candidates so far sorted by (distance, row) across its
// lanes -- lane j holds entry j in two registers -- and the K-th of them as a wave-uniform threshold.  A finished distance is
// compared with the threshold; only when some lane of the wave beats it are the winners inserted one by one (a ballot, a
// broadcast of the winner, a shift of the entries behind its place by one lane).  After the first few hundred candidates
// an insertion is rare.  At the end the four waves' lists go to LDS and one wave per query ranks the 4 K entries by
// (distance, row) and writes the first K.  The order (distance, row) is total (a row occurs once), so the K smallest are one
// set whatever the chunking, the lane a candidate lands on or the order of the insertions: the output does not depend on the
// launch geometry, and admission is applied per candidate before the comparison.
#include "common.h"

#include <climits>

namespace {

constexpr int AN_THREADS = 256, AN_WAVES = AN_THREADS / 64;
constexpr int AN_CT = 3;                                   // candidates per lane and chunk
constexpr int AN_CHUNK = AN_THREADS * AN_CT;               // candidates per staged chunk
constexpr int AN_QT = 4;                                   // queries per block
constexpr int AN_MAX_M = TECM_ANALOG_MAX_M, AN_MAX_K = TECM_ANALOG_MAX_K;
constexpr int AN_ROWS = AN_CHUNK + AN_MAX_M;               // staged rows: a chunk and its halo of at most m - 1 = 511

static_assert(AN_MAX_K <= 64, "a wave's list holds one entry per lane");

struct AnalogSearchArgs {
  TecmAnalogSearch s;
  int32_t ncand, tiles;                                    // valid candidates 0 .. ncand - 1; query tiles per node
};

// (d0, c0) before (d1, c1): by distance, the earlier archive row on equal distance
__device__ __forceinline__ bool an_before(float d0, int c0, float d1, int c1) { return d0 < d1 || (d0 == d1 && c0 < c1); }

__device__ __forceinline__ float an_readlane(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__global__ __launch_bounds__(AN_THREADS) void analog_search_kernel(AnalogSearchArgs a) {
  __shared__ float a_lds[AN_ROWS];
  __shared__ __attribute__((aligned(16))) float q_lds[AN_QT][AN_MAX_M];
  __shared__ float m_d[AN_QT][AN_WAVES * AN_MAX_K];
  __shared__ int m_c[AN_QT][AN_WAVES * AN_MAX_K];
  const TecmAnalogSearch& s = a.s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x / a.tiles;
  const int q0 = (blockIdx.x - n * a.tiles) * AN_QT;
  const int m = s.m, K = s.K;
  const int64_t Ta = s.Ta;
  const float inf = __builtin_inff();
  const bool keyed = s.key_arch != nullptr;

  // the tile's query segments; a query past S, or one whose window leaves Xq, is all NaN and selects nothing
  const int64_t qrow = (int64_t)s.N * s.C;
  for (int e = tid; e < AN_QT * m; e += AN_THREADS) {
    const int q = e / m, l = e - q * m;
    float v = __builtin_nanf("");
    if (q0 + q < s.S) {
      const int64_t start = s.starts[q0 + q];
      if (start >= 0 && start + s.L_in <= s.Tq) v = s.Xq[(start + s.L_in - m + l) * qrow + (int64_t)n * s.C + s.channel];
    }
    q_lds[q][l] = v;
  }
  int kq[AN_QT];
  int64_t oq[AN_QT];
#pragma unroll
  for (int q = 0; q < AN_QT; ++q) {
    const int sq = q0 + q < s.S ? q0 + q : s.S - 1;
    kq[q] = keyed ? s.key_q[sq] : 0;
    oq[q] = s.starts[sq] + s.L_in + s.origin_shift;
  }

  float ld[AN_QT], thr_d[AN_QT];                           // the wave's lists, entry `lane`, and their K-th entries
  int lc[AN_QT], thr_c[AN_QT];
#pragma unroll
  for (int q = 0; q < AN_QT; ++q) {
    ld[q] = thr_d[q] = inf;
    lc[q] = thr_c[q] = INT_MAX;
  }

  const float* arch = s.A + (int64_t)n * Ta;
  for (int c0 = 0; c0 < a.ncand; c0 += AN_CHUNK) {
    __syncthreads();                                       // the previous chunk has been consumed (first trip: q_lds is complete)
    for (int r = tid; r < AN_CHUNK + m - 1; r += AN_THREADS) a_lds[r] = (int64_t)c0 + r < Ta ? arch[c0 + r] : 0.0f;
    __syncthreads();
    if (c0 + wave * 64 >= a.ncand) continue;               // wave-uniform: none of this wave's candidates exists

    float acc[AN_QT][AN_CT];
#pragma unroll
    for (int q = 0; q < AN_QT; ++q)
#pragma unroll
      for (int j = 0; j < AN_CT; ++j) acc[q][j] = 0.0f;
    int l = 0;
    for (; l + 4 <= m; l += 4) {
      float av[AN_CT][4];
#pragma unroll
      for (int j = 0; j < AN_CT; ++j)
#pragma unroll
        for (int u = 0; u < 4; ++u) av[j][u] = a_lds[j * AN_THREADS + tid + l + u];
#pragma unroll
      for (int q = 0; q < AN_QT; ++q) {
        const float4 qv = *reinterpret_cast<const float4*>(&q_lds[q][l]);
        const float qs[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int j = 0; j < AN_CT; ++j)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float t = av[j][u] - qs[u];
            acc[q][j] = fmaf(t, t, acc[q][j]);
          }
      }
    }
    for (; l < m; ++l) {
      float av[AN_CT];
#pragma unroll
      for (int j = 0; j < AN_CT; ++j) av[j] = a_lds[j * AN_THREADS + tid + l];
#pragma unroll
      for (int q = 0; q < AN_QT; ++q) {
        const float qv = q_lds[q][l];
#pragma unroll
        for (int j = 0; j < AN_CT; ++j) {
          const float t = av[j] - qv;
          acc[q][j] = fmaf(t, t, acc[q][j]);
        }
      }
    }

#pragma unroll
    for (int j = 0; j < AN_CT; ++j) {
      const int c = c0 + j * AN_THREADS + tid;
      const bool valid = c < a.ncand;
      const int key = keyed && valid ? s.key_arch[c + m] : 0;
#pragma unroll
      for (int q = 0; q < AN_QT; ++q) {
        const float d = acc[q][j];
        bool ok = valid && d < inf && (!keyed || key == kq[q]);          // d < inf: neither NaN nor an overflowed sum
        if (s.exclude > 0) {
          const int64_t gap = (int64_t)c + m - oq[q];
          ok = ok && (gap < 0 ? -gap : gap) >= s.exclude;
        }
        ok = ok && an_before(d, c, thr_d[q], thr_c[q]);
        unsigned long long mask = __ballot(ok);
        while (mask) {
          const int src = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          const float nd = an_readlane(d, src);
          const int nc = __builtin_amdgcn_readlane(c, src);
          if (!an_before(nd, nc, thr_d[q], thr_c[q])) continue;           // an earlier insertion has tightened the threshold
          const int p = __popcll(__ballot(an_before(ld[q], lc[q], nd, nc)));          // the entries before the newcomer: lanes 0 .. p - 1
          const float ud = __shfl_up(ld[q], 1);
          const int uc = __shfl_up(lc[q], 1);
          if (lane == p) {
            ld[q] = nd;
            lc[q] = nc;
          } else if (lane > p) {
            ld[q] = ud;
            lc[q] = uc;
          }
          thr_d[q] = an_readlane(ld[q], K - 1);
          thr_c[q] = __builtin_amdgcn_readlane(lc[q], K - 1);
        }
      }
    }
  }

  // the four lists of a query -> its K smallest by (distance, row)
  __syncthreads();
#pragma unroll
  for (int q = 0; q < AN_QT; ++q)
    if (lane < K) {
      m_d[q][wave * K + lane] = ld[q];
      m_c[q][wave * K + lane] = lc[q];
    }
  __syncthreads();
  const int E = AN_WAVES * K;                              // <= 128: two entries per lane
  for (int q = wave; q < AN_QT; q += AN_WAVES) {
    const int sq = q0 + q;
    if (sq >= s.S) continue;                               // wave-uniform
    const int e0 = lane, e1 = lane + 64;
    const float d0 = e0 < E ? m_d[q][e0] : inf, d1 = e1 < E ? m_d[q][e1] : inf;
    const int c0 = e0 < E ? m_c[q][e0] : INT_MAX, c1 = e1 < E ? m_c[q][e1] : INT_MAX;
    int r0 = 0, r1 = 0;
    for (int i = 0; i < E; ++i) {
      const float di = m_d[q][i];
      const int ci = m_c[q][i];
      r0 += an_before(di, ci, d0, c0) ? 1 : 0;
      r1 += an_before(di, ci, d1, c1) ? 1 : 0;
    }
    const bool real0 = d0 < inf, real1 = d1 < inf;         // an unused entry is (+inf, INT_MAX)
    const int found = __popcll(__ballot(real0)) + __popcll(__ballot(real1));
    const int cnt = found < K ? found : K;
    const int64_t cell = (int64_t)sq * s.N + n;
    int32_t* idx = s.idx + cell * K;
    float* dist = s.dist + cell * K;
    if (real0 && r0 < K) {
      idx[r0] = c0;
      dist[r0] = d0;
    }
    if (real1 && r1 < K) {
      idx[r1] = c1;
      dist[r1] = d1;
    }
    if (lane < K && lane >= cnt) {
      idx[lane] = -1;
      dist[lane] = inf;
    }
    if (lane == 0) s.count[cell] = cnt;
  }
}

// ------------------------------------------------------------------ forecast: gather and mean
// One thread per (window, horizon, node), lanes along nodes: the stores run along the node-contiguous outputs, the loads are
// the gather.  The mean is one fp64 sum over the `count` members in ascending k, divided once and rounded to fp32.
__global__ __launch_bounds__(256) void analog_forecast_kernel(TecmAnalogForecast f, int tiles) {
  const int tile = blockIdx.x % tiles;
  const int bh = blockIdx.x / tiles;
  const int b = bh / f.L_out, h = bh - b * f.L_out;
  const int n = tile * 256 + threadIdx.x;
  if (n >= f.N) return;
  const int64_t cell = (int64_t)b * f.N + n;
  int cnt = f.count[cell];
  cnt = cnt < 0 ? 0 : (cnt > f.K ? f.K : cnt);
  const int32_t* idx = f.idx + cell * f.K;
  const float* y = f.Y + (int64_t)n * f.Ty;
  const float nan = __builtin_nanf("");
  double sum = 0.0;
  for (int k = 0; k < f.K; ++k) {
    float v = nan;
    if (k < cnt) {
      const int64_t r = (int64_t)idx[k] + f.m + h;
      if (idx[k] >= 0 && r < f.Ty) v = y[r];               // never read outside the series
      sum += (double)v;
    }
    if (f.members) f.members[(((int64_t)k * f.B + b) * f.L_out + h) * f.N + n] = v;
  }
  if (f.out) f.out[b * f.o_stride_b + h * f.o_stride_h + n * f.o_stride_n] = cnt > 0 ? (float)(sum / (double)cnt) : nan;
}

// ------------------------------------------------------------------ host side
// Validates the shape of a search (pointers are not looked at) and fills the launch geometry; returns an error text or nullptr.
const char* analog_search_args(const TecmAnalogSearch* s, AnalogSearchArgs* a) {
  if (!s) return "null descriptor";
  if (s->K < 1 || s->K > TECM_ANALOG_MAX_K) return "K must lie in [1, 32]";
  if (s->L_in < 1) return "L_in must be positive";
  if (s->m < 1 || s->m > TECM_ANALOG_MAX_M) return "m must lie in [1, 512]";
  if (s->m > s->L_in) return "m reaches before the input window (m > L_in)";
  if (s->L_out < 1 || s->L_out > TECM_ANALOG_MAX_H) return "L_out must lie in [1, 32]";
  if (s->N < 1 || s->C < 1 || s->S < 1 || s->Ta < 1 || s->Ty < 1 || s->Tq < 1) return "bad shape";
  if (s->channel < 0 || s->channel >= s->C) return "channel lies outside [0, C)";
  if (s->Ta > 0x7ffff000LL || s->Ty > 0x7ffff000LL || s->Tq > 0x7ffff000LL) return "a series longer than 2^31 - 4096 rows";
  if (s->L_in > s->Tq) return "the query series is shorter than L_in";
  if (s->exclude < 0) return "exclude must not be negative";
  int64_t ncand = (s->Ta < s->Ty - s->L_out ? s->Ta : s->Ty - s->L_out) - s->m + 1;
  if (ncand < 0) ncand = 0;
  if (s->key_arch && ncand > 0 && s->Tk < ncand + s->m) return "key_arch is shorter than the last candidate's origin row (Tk)";
  a->s = *s;
  a->ncand = (int32_t)ncand;
  a->tiles = (s->S + AN_QT - 1) / AN_QT;
  if ((int64_t)a->tiles * s->N > 0x7fffffffLL) return "too many (node, query tile) pairs for one launch";
  return nullptr;
}

}  // namespace

extern "C" int tecm_analog_search_supported(const TecmAnalogSearch* s, int32_t* chunk, int32_t* query_tile, int64_t* n_candidates) {
  AnalogSearchArgs a;
  const char* bad = analog_search_args(s, &a);
  if (bad) {
    tecm_set_error("tecm_analog_search: %s", bad);
    return 0;
  }
  if (chunk) *chunk = AN_CHUNK;
  if (query_tile) *query_tile = AN_QT;
  if (n_candidates) *n_candidates = a.ncand;
  return 1;
}

extern "C" int tecm_analog_search(const TecmAnalogSearch* s, void* stream) {
  AnalogSearchArgs a;
  const char* bad = analog_search_args(s, &a);
  TECM_REQUIRE(!bad, TECM_E_ARG, "tecm_analog_search: %s", bad);
  TECM_REQUIRE(s->A && s->Xq && s->starts && s->idx && s->dist && s->count, TECM_E_ARG, "tecm_analog_search: null pointer");
  TECM_REQUIRE((s->key_arch != nullptr) == (s->key_q != nullptr), TECM_E_ARG,
               "tecm_analog_search: key_arch and key_q must be given together");
  if (s->starts_host_check) {
    for (int b = 0; b < s->S; ++b) {
      const int64_t s0 = s->starts_host_check[b];
      TECM_REQUIRE(s0 >= 0 && s0 + s->L_in <= s->Tq, TECM_E_ARG,
                   "tecm_analog_search: window %d starts at %lld, outside [0, Tq - L_in]", b, (long long)s0);
    }
  }
  hipLaunchKernelGGL(analog_search_kernel, dim3((unsigned)(a.tiles * s->N)), dim3(AN_THREADS), 0, (hipStream_t)stream, a);
  TECM_CHECK_LAUNCH("tecm_analog_search");
  return TECM_OK;
}

extern "C" int tecm_analog_forecast(const TecmAnalogForecast* f, void* stream) {
  TECM_REQUIRE(f, TECM_E_ARG, "tecm_analog_forecast: null descriptor");
  TECM_REQUIRE(f->Y && f->idx && f->count && (f->out || f->members), TECM_E_ARG, "tecm_analog_forecast: null pointer");
  TECM_REQUIRE(f->K >= 1 && f->K <= TECM_ANALOG_MAX_K, TECM_E_ARG, "tecm_analog_forecast: K must lie in [1, 32]");
  TECM_REQUIRE(f->m >= 1 && f->m <= TECM_ANALOG_MAX_M, TECM_E_ARG, "tecm_analog_forecast: m must lie in [1, 512]");
  TECM_REQUIRE(f->L_out >= 1 && f->L_out <= TECM_ANALOG_MAX_H, TECM_E_ARG, "tecm_analog_forecast: L_out must lie in [1, 32]");
  TECM_REQUIRE(f->N >= 1 && f->B >= 1 && f->Ty >= 1 && f->Ty <= 0x7ffff000LL, TECM_E_ARG, "tecm_analog_forecast: bad shape");
  TECM_REQUIRE(!f->out || f->L_out == 1 || f->o_stride_h != 0, TECM_E_ARG, "tecm_analog_forecast: needs a non-zero horizon stride");
  const int tiles = (f->N + 255) / 256;
  TECM_REQUIRE((int64_t)tiles * f->B * f->L_out <= 0x7fffffffLL, TECM_E_ARG, "tecm_analog_forecast: too many windows for one launch");
  hipLaunchKernelGGL(analog_forecast_kernel, dim3((unsigned)(tiles * f->B * f->L_out)), dim3(256), 0, (hipStream_t)stream, *f, tiles);
  TECM_CHECK_LAUNCH("tecm_analog_forecast");
  return TECM_OK;
}
