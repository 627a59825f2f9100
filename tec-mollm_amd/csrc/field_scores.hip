// Multivariate scores of a K-member ensemble per (sample, horizon): tecm_field_scores (include/tecmollm.h (3m)), the kernels
// under FieldMetrics (src/evaluation/metrics.py) -- the energy score and the variogram score by pair class, the two scores
// that see whether a member is a plausible MAP (tecm_ensemble_stats (3c) sorts the members of every cell and is blind to it).
//
// Five launches, no atomics on the sums, every order fixed:
//   field_energy_kernel        block (split, h, s), 256 threads.  The K + 1 vectors x_0 .. x_{K-1}, y of a chunk of 128 nodes are
//                              staged in LDS as [node][vector] (row length odd: lanes that read different vectors of one node hit
//                              different banks).  A thread owns up to 9 of the K (K + 1) / 2 + 1 sums of squares -- one per
//                              pair of vectors, and the one of (mean_k x_k) - y -- and adds its nodes in ascending order in
//                              float64; the chunks c = split, split + NS, ... of a block go into the same registers.  The
//                              differences x_k - x_k' are taken in float64 straight from the float32 values (they are exact
//                              there), which is the deviation form ||d_k - d_k'|| of the header without its extra rounding.
//   field_pairs_kernel<ORDER>  block (tile pair p = (ti <= tj), h, s), 256 threads.  The K + 1 fields of the T row nodes and the T
//                              column nodes are staged in LDS as [field][node] after the value pipeline.  Lanes run along the
//                              columns j (one byte of pair_class per lane, consecutive in memory), a wave walks rows four at a
//                              time: per member one conflict-free column read and one 16-byte broadcast row read feed four
//                              pair terms (float32: difference, v_sqrt_f32 -- 1 ulp --, k-ascending sum, one division).  The
//                              class of a pair is a run-time index, so a thread's per-class sums live in a column of LDS that
//                              only it touches ([class][sum][thread], float64; counts uint32) -- no scratch.  At the end the 256
//                              columns of a (class, sum) cell are added in four ascending quarters and the quarters in order.
//   field_energy_sample_kernel block (h, s): the square roots (float64) of the pair sums, splits added in ascending order; A
//                              and D per thread in ascending pair order, then thread 0 adds the 256 partials in ascending order.
//   field_pairs_sample_kernel  thread (s, h, class, sum): the tile pairs in ascending p.
//   field_cells_kernel         thread (g, h) or (g, h, class): the samples of group g in ascending s, then ONE read-modify-write
//                              of the cell's statistics; a group that does not occur touches nothing; thread 0 reports bad ids.
// A sample whose group id is outside [0, G) is dropped by every kernel (its partials are never written and never read).
//
// The LDS accumulators (28 bytes per thread and class) are what bounds the pair kernel's occupancy: 56 KiB at NB = 8, so two
// blocks = 8 waves per CU next to 17 KiB of fields at K = 16.  The inner loop is bound by the square roots, not by latency.
#include "common.h"
#include "metrics_value.h"

namespace {

constexpr int FS_THREADS = TECM_FIELD_THREADS;
constexpr int FS_ECHUNK = 128;                       // nodes per staged chunk of the energy kernel
constexpr int FS_ESLOTS = 9;                         // ceil((64 * 65 / 2 + 1) / 256): sums of squares per thread at K = 64
constexpr int64_t FS_ACC_BYTES = 3 * 8 + 4;          // per thread and class: sum e^2, sum v_o, sum v_e (float64), pairs (uint32)
constexpr int64_t FS_LDS_BUDGET = 160 * 1024;
static_assert(FS_ESLOTS * FS_THREADS >= TECM_ENS_MAX_K * (TECM_ENS_MAX_K + 1) / 2 + 1, "energy slots");
static_assert(TECM_FIELD_MAX_CLASSES * 16 <= FS_THREADS, "one thread per (class, sum, quarter)");

struct FieldGeo {
  int T;                    // nodes per tile of the pair kernel
  int64_t nt, P;            // tiles, tile pairs ti <= tj
  int64_t ne;               // chunks of the energy kernel
  int NS;                   // blocks per (s, h) of the energy kernel
  int64_t P2;               // sums of squares per (s, h): K (K + 1) / 2 pairs of vectors and (mean - y)
  int64_t lds_pairs, lds_energy;
  int64_t off_vpart, off_es, off_vs, ws_doubles;      // workspace, in doubles: [energy partials | pair partials | es | vs]
};

int64_t pairs_lds(int T, int K, int NB) {
  return (int64_t)(K + 1) * 2 * T * 4 + (int64_t)NB * FS_THREADS * FS_ACC_BYTES + FS_THREADS * 8;
}

// pure host arithmetic; sets tecm_last_error and returns false on a shape that is not served
bool field_geometry(const char* who, int64_t S, int32_t H, int64_t I, int32_t K, int32_t NB, FieldGeo* g) {
  if (!(S > 0 && H > 0 && I > 0)) { tecm_set_error("%s: bad shape", who); return false; }
  if (!(K >= 1 && K <= TECM_ENS_MAX_K)) { tecm_set_error("%s: K = %d outside [1, %d]", who, (int)K, TECM_ENS_MAX_K); return false; }
  if (!(NB >= 0 && NB <= TECM_FIELD_MAX_CLASSES)) {
    tecm_set_error("%s: NB = %d outside [0, %d]", who, (int)NB, TECM_FIELD_MAX_CLASSES);
    return false;
  }
  if (S > TECM_FIELD_MAX_GRID || H > TECM_FIELD_MAX_GRID) {
    tecm_set_error("%s: S and H must be <= %d (grid dimensions)", who, TECM_FIELD_MAX_GRID);
    return false;
  }
  g->T = pairs_lds(128, K, NB) <= FS_LDS_BUDGET ? 128 : 64;
  g->lds_pairs = pairs_lds(g->T, K, NB);
  if (g->lds_pairs > FS_LDS_BUDGET) { tecm_set_error("%s: %lld bytes of LDS", who, (long long)g->lds_pairs); return false; }
  g->nt = (I + g->T - 1) / g->T;
  if (g->nt > TECM_FIELD_MAX_TILES) {
    tecm_set_error("%s: I = %lld gives more than %d tiles of %d nodes", who, (long long)I, TECM_FIELD_MAX_TILES, g->T);
    return false;
  }
  g->P = g->nt * (g->nt + 1) / 2;                     // < 2^31 by the tile limit
  g->ne = (I + FS_ECHUNK - 1) / FS_ECHUNK;
  g->NS = (int)(g->ne < TECM_FIELD_ENERGY_SPLITS ? g->ne : TECM_FIELD_ENERGY_SPLITS);
  g->P2 = (int64_t)K * (K + 1) / 2 + 1;
  g->lds_energy = (int64_t)FS_ECHUNK * ((K + 1) | 1) * 4;
  const int64_t SH = S * H;                           // < 2^32
  g->off_vpart = SH * g->NS * g->P2;                  // < 2^32 * 8 * 2081
  const int64_t per_sh = g->P * NB * 4;               // < 2^31 * 64
  if (per_sh > (INT64_MAX / 16) / SH) { tecm_set_error("%s: the workspace does not fit 64-bit addressing", who); return false; }
  g->off_es = g->off_vpart + SH * per_sh;
  g->off_vs = g->off_es + SH * 3;
  g->ws_doubles = g->off_vs + SH * NB * 4;
  return true;
}

__device__ __forceinline__ float field_member(const TecmFieldScores& q, int k, int64_t s, int64_t h, int64_t i) {
  float p = q.members[(int64_t)k * q.m_stride_k + s * q.m_stride_s + h * q.m_stride_h + i * q.m_stride_i];
  if (!isfinite(p)) p = 0.f;
  p = nan_to_num_tec(unscale_f32(p, q.mean, q.scale));
  if (q.clip) p = fminf(fmaxf(p, q.clip_lo), q.clip_hi);
  return p;
}
__device__ __forceinline__ float field_truth(const TecmFieldScores& q, int64_t s, int64_t h, int64_t i) {
  return nan_to_num_tec(unscale_f32(q.target[s * q.t_stride_s + h * q.t_stride_h + i * q.t_stride_i], q.mean, q.scale));
}
__device__ __forceinline__ bool field_sample_ok(const TecmFieldScores& q, int64_t s) {
  const int id = q.group ? q.group[s] : 0;
  return (unsigned)id < (unsigned)q.G;
}

template <int ORDER>
__device__ __forceinline__ float vario(float a, float b) {
  const float d = fabsf(a - b);
  if constexpr (ORDER == TECM_FIELD_ORDER_HALF) return __builtin_amdgcn_sqrtf(d);
  else if constexpr (ORDER == TECM_FIELD_ORDER_ONE) return d;
  else return d * d;
}

// ------------------------------------------------------------------------------------------------ variogram: the pairs
template <int ORDER>
__global__ __launch_bounds__(FS_THREADS) void field_pairs_kernel(TecmFieldScores q, int T, int64_t nt, int64_t P, double* part) {
  extern __shared__ __align__(16) unsigned char fs_smem[];
  const int t = threadIdx.x;
  const int64_t s = blockIdx.z, h = blockIdx.y, p = blockIdx.x;
  if (!field_sample_ok(q, s)) return;                                   // block-uniform
  int64_t ti = 0, rem = p, row = nt;
  while (rem >= row) { rem -= row; --row; ++ti; }
  const int64_t tj = ti + rem;
  const bool diag = ti == tj;
  const int K = q.K, F = K + 1, NB = q.NB, W = 2 * T;
  float* fld = reinterpret_cast<float*>(fs_smem);                       // [F][W]: row tile | column tile
  double* acc = reinterpret_cast<double*>(fs_smem + (size_t)F * W * 4); // [NB][3][threads]
  uint32_t* cnt = reinterpret_cast<uint32_t*>(acc + NB * 3 * FS_THREADS);   // [NB][threads]
  double* red = reinterpret_cast<double*>(cnt + NB * FS_THREADS);       // [threads]

  for (int idx = t; idx < F * W; idx += FS_THREADS) {
    const int f = idx / W, n = idx - f * W;
    const int64_t i = n < T ? ti * T + n : tj * T + (n - T);
    float v = 0.f;
    if (i < q.I && !(diag && n >= T)) v = f < K ? field_member(q, f, s, h, i) : field_truth(q, s, h, i);
    fld[idx] = v;
  }
  for (int c = 0; c < NB; ++c) {
    acc[(c * 3 + 0) * FS_THREADS + t] = 0.0;
    acc[(c * 3 + 1) * FS_THREADS + t] = 0.0;
    acc[(c * 3 + 2) * FS_THREADS + t] = 0.0;
    cnt[c * FS_THREADS + t] = 0u;
  }
  __syncthreads();

  const int b = t & (T - 1), rg = t / T;                                // column of the lane; row group of the wave
  const int rows_per = T / (FS_THREADS / T);
  const int colbase = diag ? 0 : T;
  const int64_t j = tj * T + b;
  const bool jin = j < q.I;
  const float Kf = (float)K;
  for (int a0 = rg * rows_per; a0 < (rg + 1) * rows_per; a0 += 4) {
    int cls[4];
    bool any = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = ti * T + a0 + r;
      cls[r] = (jin && i < j) ? (int)q.pair_class[i * q.I + j] : 255;   // i < j < I: above the diagonal and in range
      any |= cls[r] < NB;
    }
    if (!any) continue;
    float ve[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; ++k) {
      const float xb = fld[k * W + colbase + b];
      const float4 xa = *reinterpret_cast<const float4*>(&fld[k * W + a0]);
      ve[0] += vario<ORDER>(xa.x, xb);
      ve[1] += vario<ORDER>(xa.y, xb);
      ve[2] += vario<ORDER>(xa.z, xb);
      ve[3] += vario<ORDER>(xa.w, xb);
    }
    const float yb = fld[K * W + colbase + b];
    const float4 ya = *reinterpret_cast<const float4*>(&fld[K * W + a0]);
    const float vo[4] = {vario<ORDER>(ya.x, yb), vario<ORDER>(ya.y, yb), vario<ORDER>(ya.z, yb), vario<ORDER>(ya.w, yb)};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (cls[r] < NB) {
        const float vef = ve[r] / Kf;
        const double e = (double)vo[r] - (double)vef;
        const int c = cls[r];
        acc[(c * 3 + 0) * FS_THREADS + t] += e * e;
        acc[(c * 3 + 1) * FS_THREADS + t] += (double)vo[r];
        acc[(c * 3 + 2) * FS_THREADS + t] += (double)vef;
        cnt[c * FS_THREADS + t] += 1u;
      }
    }
  }
  __syncthreads();
  // cell = (class, sum) with sum 0 = pairs, 1 = e^2, 2 = v_o, 3 = v_e; four threads per cell add a quarter of the columns each
  const int cells = NB * 4;
  if (t < cells * 4) {
    const int cell = t >> 2, c = cell >> 2, st = cell & 3, u0 = (t & 3) * (FS_THREADS / 4);
    double sum = 0.0;
    for (int u = u0; u < u0 + FS_THREADS / 4; ++u)
      sum += st == 0 ? (double)cnt[c * FS_THREADS + u] : acc[(c * 3 + st - 1) * FS_THREADS + u];
    red[t] = sum;
  }
  __syncthreads();
  if (t < cells * 4 && (t & 3) == 0)
    part[((s * q.H + h) * P + p) * cells + (t >> 2)] = ((red[t] + red[t + 1]) + red[t + 2]) + red[t + 3];
}

__global__ __launch_bounds__(FS_THREADS) void field_pairs_sample_kernel(TecmFieldScores q, int64_t P, const double* part,
                                                                        double* vs_sample) {
  const int64_t cells = (int64_t)q.NB * 4;
  const int64_t id = (int64_t)blockIdx.x * FS_THREADS + threadIdx.x;
  if (id >= q.S * q.H * cells) return;
  const int64_t sh = id / cells, cell = id - sh * cells;
  if (!field_sample_ok(q, sh / q.H)) return;
  const double* src = part + sh * P * cells + cell;
  double sum = 0.0;
  for (int64_t p = 0; p < P; ++p) sum += src[p * cells];
  vs_sample[id] = sum;
  if (q.vs_out) q.vs_out[id] = sum;
}

// ------------------------------------------------------------------------------------------------ energy: the norms
// the pair (a < b) of the K + 1 vectors with number qi, rows a = 0, 1, ... holding b = a + 1 .. K
__device__ __forceinline__ void energy_pair(int qi, int K, int& a, int& b) {
  int len = K;
  a = 0;
  while (qi >= len) { qi -= len; --len; ++a; }
  b = a + 1 + qi;
}

__global__ __launch_bounds__(FS_THREADS) void field_energy_kernel(TecmFieldScores q, int64_t ne, int NS, int P2, double* part) {
  extern __shared__ __align__(16) unsigned char fs_smem[];
  float* xs = reinterpret_cast<float*>(fs_smem);                        // [FS_ECHUNK][FP]
  const int t = threadIdx.x;
  const int64_t s = blockIdx.z, h = blockIdx.y;
  const int split = blockIdx.x;
  if (!field_sample_ok(q, s)) return;                                   // block-uniform
  const int K = q.K, F = K + 1, FP = F | 1;
  const double dK = (double)K;
  int pa[FS_ESLOTS], pb[FS_ESLOTS];                                      // statically indexed: every slot loop is unrolled
  double acc[FS_ESLOTS];
#pragma unroll
  for (int sl = 0; sl < FS_ESLOTS; ++sl) {
    const int qi = t + sl * FS_THREADS;
    acc[sl] = 0.0;
    pa[sl] = -2;                                                         // no sum in this slot
    pb[sl] = 0;
    if (qi < P2 - 1) energy_pair(qi, K, pa[sl], pb[sl]);
    else if (qi == P2 - 1) pa[sl] = -1;                                  // (mean_k x_k) - y
  }
  for (int64_t c = split; c < ne; c += NS) {
    const int64_t i0 = c * FS_ECHUNK;
    const int nn = (int)((q.I - i0) < FS_ECHUNK ? (q.I - i0) : FS_ECHUNK);
    __syncthreads();                                                     // the previous chunk has been consumed
    for (int idx = t; idx < F * FS_ECHUNK; idx += FS_THREADS) {
      const int f = idx / FS_ECHUNK, n = idx - f * FS_ECHUNK;
      if (n < nn) xs[n * FP + f] = f < K ? field_member(q, f, s, h, i0 + n) : field_truth(q, s, h, i0 + n);
    }
    __syncthreads();
#pragma unroll
    for (int sl = 0; sl < FS_ESLOTS; ++sl) {
      double sum = acc[sl];
      if (pa[sl] >= 0) {
        const int a = pa[sl], b = pb[sl];
        for (int n = 0; n < nn; ++n) {
          const double d = (double)xs[n * FP + a] - (double)xs[n * FP + b];
          sum += d * d;
        }
      } else if (pa[sl] == -1) {
        for (int n = 0; n < nn; ++n) {
          double mu = 0.0;
          for (int k = 0; k < K; ++k) mu += (double)xs[n * FP + k];
          const double e = mu / dK - (double)xs[n * FP + K];
          sum += e * e;
        }
      }
      acc[sl] = sum;
    }
  }
  double* dst = part + ((s * q.H + h) * NS + split) * (int64_t)P2;
#pragma unroll
  for (int sl = 0; sl < FS_ESLOTS; ++sl) {
    const int qi = t + sl * FS_THREADS;
    if (qi < P2) dst[qi] = acc[sl];
  }
}

__global__ __launch_bounds__(FS_THREADS) void field_energy_sample_kernel(TecmFieldScores q, int NS, int P2, const double* part,
                                                                         double* es_sample) {
  __shared__ double sA[FS_THREADS], sD[FS_THREADS];
  __shared__ double sE;
  const int t = threadIdx.x, K = q.K;
  const int64_t h = blockIdx.x, s = blockIdx.y;
  if (!field_sample_ok(q, s)) return;                                   // block-uniform
  const double* src = part + (s * q.H + h) * NS * (int64_t)P2;
  double A = 0.0, D = 0.0;
  for (int qi = t; qi < P2; qi += FS_THREADS) {
    double tot = 0.0;
    for (int sp = 0; sp < NS; ++sp) tot += src[(int64_t)sp * P2 + qi];
    const double r = sqrt(tot);
    if (qi == P2 - 1) {
      sE = r;
    } else {
      int a, b;
      energy_pair(qi, K, a, b);
      if (b == K) A += r;                                                // ||x_a - y||
      else D += r;                                                       // ||x_a - x_b||
    }
  }
  sA[t] = A;
  sD[t] = D;
  __syncthreads();
  if (t == 0) {
    double a = 0.0, d = 0.0;
    for (int u = 0; u < FS_THREADS; ++u) { a += sA[u]; d += sD[u]; }
    double* o = es_sample + (s * q.H + h) * 3;
    o[0] = a / (double)K; o[1] = d; o[2] = sE;
    if (q.es_out) {
      double* e = q.es_out + (s * q.H + h) * 3;
      e[0] = o[0]; e[1] = d; e[2] = sE;
    }
  }
}

// ------------------------------------------------------------------------------------------------ the cells (g, h[, class])
__global__ __launch_bounds__(FS_THREADS) void field_cells_kernel(TecmFieldScores q, const double* es_sample, const double* vs_sample) {
  const int64_t per = 1 + q.NB;
  const int64_t id = (int64_t)blockIdx.x * FS_THREADS + threadIdx.x;
  if (id >= (int64_t)q.G * q.H * per) return;
  const int64_t gh = id / per, j = id - gh * per, h = gh % q.H;
  const int g = (int)(gh / q.H);
  double n = 0.0, v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  bool bad = false;
  for (int64_t s = 0; s < q.S; ++s) {
    const int gid = q.group ? q.group[s] : 0;
    if ((unsigned)gid >= (unsigned)q.G) bad = true;
    if (gid != g) continue;
    n += 1.0;
    if (j == 0) {
      const double* e = es_sample + (s * q.H + h) * 3;
      v0 += e[0]; v1 += e[1]; v2 += e[2];
    } else {
      const double* v = vs_sample + ((s * q.H + h) * q.NB + (j - 1)) * 4;
      v0 += v[0]; v1 += v[1]; v2 += v[2]; v3 += v[3];
    }
  }
  if (bad && id == 0) atomicOr(q.err_flag, TECM_BAD_GROUP);
  if (n == 0.0) return;                                                  // the group does not occur: nothing is touched
  if (j == 0) {
    double* o = q.es_stats + gh * TECM_FIELD_ES_STATS;
    o[0] += n; o[1] += v0; o[2] += v1; o[3] += v2;
  } else {
    double* o = q.vs_stats + (gh * q.NB + (j - 1)) * TECM_FIELD_VS_STATS;
    o[0] += n; o[1] += v0; o[2] += v1; o[3] += v2; o[4] += v3;
  }
}

template <int ORDER>
int launch_pairs(const TecmFieldScores* f, const FieldGeo& g, double* part, hipStream_t st) {
  static bool attr_set = false;
  if (!attr_set) {
    TECM_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(&field_pairs_kernel<ORDER>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)FS_LDS_BUDGET) == hipSuccess,
                 TECM_E_LAUNCH, "tecm_field_scores: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    attr_set = true;
  }
  hipLaunchKernelGGL(field_pairs_kernel<ORDER>, dim3((unsigned)g.P, (unsigned)f->H, (unsigned)f->S), dim3(FS_THREADS),
                     (size_t)g.lds_pairs, st, *f, g.T, g.nt, g.P, part);
  return TECM_OK;
}

}  // namespace

extern "C" int tecm_field_scores_plan(int64_t S, int32_t H, int64_t I, int32_t K, int32_t NB, int32_t* tile, int64_t* lds_bytes,
                                      int64_t* workspace_bytes) {
  FieldGeo g;
  if (!field_geometry("tecm_field_scores_plan", S, H, I, K, NB, &g)) return 0;
  if (tile) *tile = g.T;
  if (lds_bytes) *lds_bytes = NB > 0 ? g.lds_pairs : g.lds_energy;
  if (workspace_bytes) *workspace_bytes = g.ws_doubles * (int64_t)sizeof(double);
  return 1;
}

extern "C" int tecm_field_scores(const TecmFieldScores* f, void* stream) {
  TECM_REQUIRE(f, TECM_E_ARG, "tecm_field_scores: null descriptor");
  TECM_REQUIRE(f->members && f->target && f->es_stats && f->err_flag && f->workspace, TECM_E_ARG,
               "tecm_field_scores: null pointer");
  TECM_REQUIRE(f->G > 0, TECM_E_ARG, "tecm_field_scores: bad shape");
  FieldGeo g;
  if (!field_geometry("tecm_field_scores", f->S, f->H, f->I, f->K, f->NB, &g)) return TECM_E_ARG;
  TECM_REQUIRE(f->NB == 0 || (f->pair_class && f->vs_stats), TECM_E_ARG,
               "tecm_field_scores: NB = %d needs pair_class and vs_stats", (int)f->NB);
  TECM_REQUIRE(f->order == TECM_FIELD_ORDER_HALF || f->order == TECM_FIELD_ORDER_ONE || f->order == TECM_FIELD_ORDER_TWO,
               TECM_E_ARG, "tecm_field_scores: order = %d is not one of TECM_FIELD_ORDER_*", (int)f->order);
  TECM_REQUIRE(f->I <= INT64_MAX / f->I, TECM_E_ARG, "tecm_field_scores: I * I does not fit 64-bit addressing");
  TECM_REQUIRE(f->scale != 0.0, TECM_E_ARG, "tecm_field_scores: scale must be non-zero");
  TECM_REQUIRE(f->workspace_bytes >= g.ws_doubles * (int64_t)sizeof(double), TECM_E_ARG,
               "tecm_field_scores: workspace of %lld bytes, needs %lld", (long long)f->workspace_bytes,
               (long long)(g.ws_doubles * (int64_t)sizeof(double)));
  TECM_REQUIRE(tecm_aligned(f->es_stats, 8) && tecm_aligned(f->vs_stats, 8) && tecm_aligned(f->es_out, 8) &&
                   tecm_aligned(f->vs_out, 8) && tecm_aligned(f->workspace, 8),
               TECM_E_ALIGN, "tecm_field_scores: statistics, per-sample outputs and workspace must be 8-byte aligned");
  TECM_REQUIRE(tecm_aligned(f->members, 4) && tecm_aligned(f->target, 4) && tecm_aligned(f->group, 4) &&
                   tecm_aligned(f->err_flag, 4),
               TECM_E_ALIGN, "tecm_field_scores: members, target, group and err_flag must be 4-byte aligned");
  const int64_t cells = (int64_t)f->G * f->H * (1 + f->NB), sample_cells = f->S * f->H * f->NB * 4;
  TECM_REQUIRE((cells + FS_THREADS - 1) / FS_THREADS < (1LL << 31) && (sample_cells + FS_THREADS - 1) / FS_THREADS < (1LL << 31),
               TECM_E_ARG, "tecm_field_scores: more than 2^31 blocks");
  hipStream_t st = (hipStream_t)stream;
  double* ws = static_cast<double*>(f->workspace);
  double *epart = ws, *vpart = ws + g.off_vpart, *es_sample = ws + g.off_es, *vs_sample = ws + g.off_vs;
  hipLaunchKernelGGL(field_energy_kernel, dim3((unsigned)g.NS, (unsigned)f->H, (unsigned)f->S), dim3(FS_THREADS),
                     (size_t)g.lds_energy, st, *f, g.ne, g.NS, (int)g.P2, epart);
  TECM_CHECK_LAUNCH("tecm_field_scores (energy)");
  hipLaunchKernelGGL(field_energy_sample_kernel, dim3((unsigned)f->H, (unsigned)f->S), dim3(FS_THREADS), 0, st, *f, g.NS,
                     (int)g.P2, epart, es_sample);
  TECM_CHECK_LAUNCH("tecm_field_scores (energy per sample)");
  if (f->NB > 0) {
    int rc;
    if (f->order == TECM_FIELD_ORDER_HALF) rc = launch_pairs<TECM_FIELD_ORDER_HALF>(f, g, vpart, st);
    else if (f->order == TECM_FIELD_ORDER_ONE) rc = launch_pairs<TECM_FIELD_ORDER_ONE>(f, g, vpart, st);
    else rc = launch_pairs<TECM_FIELD_ORDER_TWO>(f, g, vpart, st);
    if (rc != TECM_OK) return rc;
    TECM_CHECK_LAUNCH("tecm_field_scores (pairs)");
    hipLaunchKernelGGL(field_pairs_sample_kernel, dim3((unsigned)((sample_cells + FS_THREADS - 1) / FS_THREADS)),
                       dim3(FS_THREADS), 0, st, *f, g.P, vpart, vs_sample);
    TECM_CHECK_LAUNCH("tecm_field_scores (pairs per sample)");
  }
  hipLaunchKernelGGL(field_cells_kernel, dim3((unsigned)((cells + FS_THREADS - 1) / FS_THREADS)), dim3(FS_THREADS), 0, st, *f,
                     es_sample, vs_sample);
  TECM_CHECK_LAUNCH("tecm_field_scores (cells)");
  return TECM_OK;
}
