// Forecast combination per cell (group, horizon, node): tecm_combine_moments / _solve / _apply (include/tecmollm.h (3l)),
// the kernels under tecmollm/combine.py.  A least-squares fit of the truth on M forecasts with an intercept needs the
// (M+2) x (M+2) moment matrix of z = [1, p_1 .. p_M, t] per cell and nothing else, so the fitting pass streams every batch
// once through combine_moments_kernel and the 35 000 small regressions are one launch of combine_solve_kernel at the end.
//
// combine_moments_kernel<MB> takes the block of metrics_map_kernel (csrc/metrics_map.hip): block (x, y, z) = (tile of 64
// nodes, chunk of 4 horizons, group g), lane = node, wave = horizon, ONE owning thread per cell.  It walks the samples in
// ascending s, SB at a time so that the loads of SB samples of every operand are in flight together, and adds its sums to
// `stats` once at the end: no atomics, a fixed order.  An operand with stride_h == 1, stride_i == H (the model's permuted
// view) is staged through the padded LDS tile of metrics_map_kernel when 1 < H <= TECM_MAP_LDS_MAX_H; the values that
// reach the sums are the same floats either way.
// M is served by the bucket MB = 1, 2, 4, 8 so that the (MB+2)(MB+3)/2 sums are statically indexed registers: the padded
// members read nothing, hold 0 and their sums are not stored.  Samples in flight per bucket: the sums take 6 / 10 / 21 / 55
// doubles, an operand's SB floats times MB + 1 operands come on top, so SB = 16, 16, 8, 4 keeps every bucket far from the
// register file's edge (no scratch: SPILL_CEILINGS) and the LDS of MB + 1 staged operands at 40 / 60 / 50 / 45 KiB.
//
// combine_solve_kernel<MB>: one thread per cell, the moments, the packed Cholesky factor and both substitutions in
// statically indexed registers.  combine_apply_kernel: one thread per (horizon, node), samples along the grid's z.
#include "common.h"

namespace {

constexpr int CMB_TILE = 64;                 // nodes per block = lanes of a wave
constexpr int CMB_HC = 4;                    // horizons per block = waves
constexpr int CMB_LD = CMB_HC + 1;           // padded LDS row (odd pitch: metrics_map.hip)
constexpr int CMB_MAX = TECM_COMBINE_MAX_MEMBERS;

__host__ __device__ constexpr int cmb_sb(int mb) { return mb <= 2 ? 16 : (mb == 4 ? 8 : 4); }
__host__ __device__ constexpr int cmb_slab(int mb) { return cmb_sb(mb) * CMB_TILE * CMB_LD; }   // floats per staged operand

// the chunk's columns of the tile's rows of one sample: base[r*H + h0 + c] -> slab[r*CMB_LD + c]
__device__ __forceinline__ void cmb_stage(float* slab, const float* base, int64_t H, int h0, int hc, int cnt) {
  for (int e = threadIdx.x; e < cnt * hc; e += 256) {
    const int r = e / hc, c = e - r * hc;
    slab[r * CMB_LD + c] = base[(int64_t)r * H + h0 + c];
  }
}

// operand o of the bucket: members 0 .. MB-1, then the target
template <int MB>
__device__ __forceinline__ const TecmCombineOperand& cmb_operand(const TecmCombineMoments& q, int o) {
  return o == MB ? q.target : q.member[o < CMB_MAX ? o : 0];
}

template <int MB>
__global__ __launch_bounds__(256) void combine_moments_kernel(TecmCombineMoments q, int lds_mask) {
  constexpr int SB = cmb_sb(MB), NZ = MB + 2, NT = NZ * (NZ + 1) / 2, SLAB = cmb_slab(MB);
  extern __shared__ float slab[];            // one SLAB per staged operand, in operand order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.z;
  const int h0 = blockIdx.y * CMB_HC;
  const int hc = min(CMB_HC, q.H - h0);
  const int64_t i0 = (int64_t)blockIdx.x * CMB_TILE;
  const int cnt = (int)(q.I - i0 < CMB_TILE ? q.I - i0 : CMB_TILE);
  const int64_t i = i0 + lane, h = h0 + wave;
  const bool own = lane < cnt && wave < hc;  // this thread's cell is (g, h, i)

  double a[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) a[n] = 0.0;
  double skipped = 0.0;

  bool present = false, bad = false;
  for (int64_t s0 = 0; s0 < q.S; s0 += SB) {
    int match = 0;                           // block-uniform: which of the SB samples belong to g
#pragma unroll
    for (int j = 0; j < SB; ++j) {
      if (s0 + j < q.S) {
        const int id = q.group ? q.group[s0 + j] : 0;
        if (id == g) match |= 1 << j;
        if ((unsigned)id >= (unsigned)q.G) bad = true;
      }
    }
    if (!match) continue;
    present = true;
    float v[MB + 1][SB];
#pragma unroll
    for (int o = 0; o <= MB; ++o) {          // operands read in place first: in flight while the others are staged
      const TecmCombineOperand& op = cmb_operand<MB>(q, o);
      const bool used = o == MB || o < q.M, in_lds = lds_mask >> o & 1;
#pragma unroll
      for (int j = 0; j < SB; ++j) {
        v[o][j] = 0.f;
        if (!used || in_lds || !(match >> j & 1) || !own) continue;
        v[o][j] = op.base[(s0 + j) * op.stride_s + h * op.stride_h + i * op.stride_i];
      }
    }
    if (lds_mask) {
      int slot = 0;
#pragma unroll
      for (int o = 0; o <= MB; ++o) {
        if (!(lds_mask >> o & 1)) continue;
        const TecmCombineOperand& op = cmb_operand<MB>(q, o);
#pragma unroll
        for (int j = 0; j < SB; ++j)
          if (match >> j & 1)
            cmb_stage(slab + slot * SLAB + j * CMB_TILE * CMB_LD, op.base + (s0 + j) * op.stride_s + i0 * q.H, q.H, h0, hc, cnt);
        ++slot;
      }
      __syncthreads();
      slot = 0;
#pragma unroll
      for (int o = 0; o <= MB; ++o) {
        if (!(lds_mask >> o & 1)) continue;
#pragma unroll
        for (int j = 0; j < SB; ++j)
          if ((match >> j & 1) && own) v[o][j] = slab[slot * SLAB + (j * CMB_TILE + lane) * CMB_LD + wave];
        ++slot;
      }
    }
#pragma unroll
    for (int j = 0; j < SB; ++j) {           // ascending s
      if (!(match >> j & 1) || !own) continue;
      double z[NZ];
      z[0] = 1.0;
      bool finite = true;
#pragma unroll
      for (int o = 0; o <= MB; ++o) {
        finite = finite && isfinite(v[o][j]);     // a padded member holds 0
        z[1 + o] = (double)v[o][j];
      }
      if (!finite) {
        skipped += 1.0;
        continue;
      }
      int n = 0;
#pragma unroll
      for (int r = 0; r < NZ; ++r)
#pragma unroll
        for (int c = r; c < NZ; ++c) a[n++] += z[r] * z[c];     // float32 x float32 is exact in float64
    }
    if (lds_mask) __syncthreads();           // the tiles are overwritten by the next SB samples
  }
  if (bad && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) atomicOr(q.err_flag, TECM_BAD_GROUP);
  if (!present || !own) return;
  const int mz = q.M + 2, K = mz * (mz + 1) / 2 + 1;
  double* cell = q.stats + (((int64_t)g * q.H + h) * K) * q.I + i;
  int n = 0;
#pragma unroll
  for (int r = 0; r < NZ; ++r) {
#pragma unroll
    for (int c = r; c < NZ; ++c, ++n) {      // bucket index -> index among the M + 2 stored; a padded member is not stored
      if ((r >= 1 && r <= MB && r > q.M) || (c >= 1 && c <= MB && c > q.M)) continue;
      const int rr = r == MB + 1 ? q.M + 1 : r, cc = c == MB + 1 ? q.M + 1 : c;
      const int k = rr * mz - rr * (rr - 1) / 2 + (cc - rr);
      cell[(int64_t)k * q.I] += a[n];
    }
  }
  cell[(int64_t)(K - 1) * q.I] += skipped;
}

// ------------------------------------------------------------------------------------------------ the solve
// Packed lower triangle: element (j, k), k <= j, at j*(j+1)/2 + k.
#define CMB_L(j, k) L[(j) * ((j) + 1) / 2 + (k)]

template <int MB>
__global__ __launch_bounds__(256) void combine_solve_kernel(TecmCombineSolve q) {
#pragma clang fp contract(off)
  const int64_t cells = (int64_t)q.G * q.H * q.I;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= cells) return;
  const int64_t i = idx % q.I, gh = idx / q.I;
  const int64_t h = gh % q.H, g = gh / q.H;
  const int M = q.M, mz = M + 2;
  const double* cell = q.stats + g * q.s_stride_g + h * q.s_stride_h + i * q.s_stride_i;
  // k of the stored upper triangle, row r <= column c among the M + 2
  auto at = [&](int r, int c) { return cell[(int64_t)(r * mz - r * (r - 1) / 2 + (c - r)) * q.s_stride_k]; };

  const double n = at(0, 0), st = at(0, M + 1), stt = at(M + 1, M + 1);
  double sp[MB], spt[MB], w0[MB], L[MB * (MB + 1) / 2];
  bool finite = isfinite(n) && isfinite(st) && isfinite(stt);
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    const bool used = m < M;
    sp[m] = used ? at(0, 1 + m) : 0.0;
    spt[m] = used ? at(1 + m, M + 1) : 0.0;
    w0[m] = used ? q.w0[m] : 0.0;
    finite = finite && isfinite(sp[m]) && isfinite(spt[m]);
#pragma unroll
    for (int k = 0; k <= m; ++k) {
      CMB_L(m, k) = used ? at(1 + k, 1 + m) : 0.0;
      finite = finite && isfinite(CMB_L(m, k));
    }
  }

  double w[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) w[m] = w0[m];
  double icpt = 0.0;
  int status = 0;
  unsigned dropped = 0;
  if (!finite) {
    status = TECM_COMBINE_NONFINITE;
  } else if (n == 0.0) {
    status = TECM_COMBINE_EMPTY;
  } else {
    double pbar[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) pbar[m] = sp[m] / n;
    const double tbar = st / n;
    if (n < (double)(M + 2)) {
      status = TECM_COMBINE_FEW;
    } else {
      const double rn = q.ridge * n;
      double b[MB];
#pragma unroll
      for (int m = 0; m < MB; ++m) {         // A = C + ridge n I (packed lower, in L), b = c + ridge n w0
        b[m] = (spt[m] - n * pbar[m] * tbar) + rn * w0[m];
#pragma unroll
        for (int k = 0; k <= m; ++k) {
          double c = CMB_L(m, k) - n * pbar[k] * pbar[m];
          if (k == m) c = c + rn;
          CMB_L(m, k) = c;
        }
      }
      unsigned kept = 0;
#pragma unroll
      for (int m = 0; m < MB; ++m) {         // Cholesky by columns, in member order; a dropped column is all zero
        const double diag = CMB_L(m, m);
        double piv = diag;
#pragma unroll
        for (int k = 0; k < m; ++k) piv = piv - CMB_L(m, k) * CMB_L(m, k);
        const bool keep = m < M && diag > 0.0 && piv > TECM_COMBINE_PIVOT_TOL * diag;
        if (keep) kept |= 1u << m;
        else if (m < M) dropped |= 1u << m;
        const double lmm = keep ? sqrt(piv) : 1.0;
        CMB_L(m, m) = lmm;
#pragma unroll
        for (int j = m + 1; j < MB; ++j) {
          double s = CMB_L(j, m);
#pragma unroll
          for (int k = 0; k < m; ++k) s = s - CMB_L(j, k) * CMB_L(m, k);
          CMB_L(j, m) = keep ? s / lmm : 0.0;
        }
      }
      double y[MB];
#pragma unroll
      for (int m = 0; m < MB; ++m) {         // L y = b over the kept members
        double s = b[m];
#pragma unroll
        for (int k = 0; k < m; ++k) s = s - CMB_L(m, k) * y[k];
        y[m] = (kept >> m & 1) ? s / CMB_L(m, m) : 0.0;
      }
#pragma unroll
      for (int m = MB - 1; m >= 0; --m) {    // L^T w = y
        double s = y[m];
#pragma unroll
        for (int j = m + 1; j < MB; ++j) s = s - CMB_L(j, m) * w[j];
        w[m] = (kept >> m & 1) ? s / CMB_L(m, m) : 0.0;
      }
      if (dropped) status = TECM_COMBINE_DROPPED;
    }
    double dot = 0.0;
#pragma unroll
    for (int m = 0; m < MB; ++m) dot = dot + w[m] * pbar[m];
    icpt = tbar - dot;
  }
  double* wout = q.weight + ((g * q.H + h) * M) * q.I + i;
#pragma unroll
  for (int m = 0; m < MB; ++m)
    if (m < M) wout[(int64_t)m * q.I] = w[m];
  q.intercept[idx] = icpt;
  q.status[idx] = status;
  q.dropped[idx] = (uint8_t)dropped;
}

// ------------------------------------------------------------------------------------------------ the blend
__global__ __launch_bounds__(256) void combine_apply_kernel(TecmCombineApply q) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * CMB_TILE + lane, h = (int64_t)blockIdx.y * CMB_HC + wave;
  bool bad = false;
  for (int64_t s = blockIdx.z; s < q.S; s += gridDim.z) {
    const int id = q.group ? q.group[s] : 0;
    const bool valid = (unsigned)id < (unsigned)q.G;
    bad = bad || !valid;
    if (i >= q.I || h >= q.H) continue;
    double acc = __builtin_nan("");
    if (valid) {
      acc = q.intercept[id * q.b_stride_g + h * q.b_stride_h + i * q.b_stride_i];
      const double* wp = q.weight + id * q.w_stride_g + h * q.w_stride_h + i * q.w_stride_i;
#pragma unroll
      for (int m = 0; m < CMB_MAX; ++m) {    // ascending m; static indices into the descriptor
        if (m >= q.M) continue;
        const TecmCombineOperand& op = q.member[m];
        acc += wp[(int64_t)m * q.w_stride_m] * (double)op.base[s * op.stride_s + h * op.stride_h + i * op.stride_i];
      }
    }
    q.out[s * q.o_stride_s + h * q.o_stride_h + i * q.o_stride_i] = (float)acc;
  }
  if (bad && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicOr(q.err_flag, TECM_BAD_GROUP);
}

int cmb_bucket(int M) { return M <= 1 ? 1 : (M <= 2 ? 2 : (M <= 4 ? 4 : 8)); }

}  // namespace

extern "C" int tecm_combine_moments(const TecmCombineMoments* c, void* stream) {
  TECM_REQUIRE(c, TECM_E_ARG, "tecm_combine_moments: null descriptor");
  TECM_REQUIRE(c->M >= 1 && c->M <= CMB_MAX, TECM_E_ARG, "tecm_combine_moments: M must be in [1, %d], got %d", CMB_MAX, c->M);
  for (int m = 0; m < c->M; ++m)
    TECM_REQUIRE(c->member[m].base, TECM_E_ARG, "tecm_combine_moments: null pointer (member %d)", m);
  TECM_REQUIRE(c->target.base && c->stats && c->err_flag, TECM_E_ARG, "tecm_combine_moments: null pointer");
  TECM_REQUIRE(c->S > 0 && c->H > 0 && c->I > 0 && c->G > 0, TECM_E_ARG, "tecm_combine_moments: bad shape");
  const int64_t chunks = ((int64_t)c->H + CMB_HC - 1) / CMB_HC, tiles = (c->I + CMB_TILE - 1) / CMB_TILE;
  TECM_REQUIRE(c->G <= 65535 && chunks <= 65535, TECM_E_ARG, "tecm_combine_moments: G and ceil(H / 4) must be <= 65535");
  TECM_REQUIRE(tiles < (1 << 24) && tiles * chunks < (1 << 24) && tiles * chunks * c->G < (1 << 24), TECM_E_ARG,
               "tecm_combine_moments: more than 2^24 blocks of 256 threads");
  const int64_t K = (int64_t)(c->M + 2) * (c->M + 3) / 2 + 1;
  TECM_REQUIRE(c->I <= INT64_MAX / (int64_t)sizeof(double) / K / c->H / c->G, TECM_E_ARG,
               "tecm_combine_moments: G * H * K * I doubles do not fit 64-bit addressing");
  TECM_REQUIRE(tecm_aligned(c->stats, 8) && tecm_aligned(c->group, 4) && tecm_aligned(c->err_flag, 4), TECM_E_ALIGN,
               "tecm_combine_moments: stats must be 8-byte aligned, group and err_flag 4-byte aligned");
  const bool lds_h = c->H > 1 && c->H <= TECM_MAP_LDS_MAX_H && c->I > 1;
  int lds_mask = 0, staged = 0;
  const int mb = cmb_bucket(c->M);
  for (int o = 0; o <= c->M; ++o) {          // bit o < MB: member o; bit MB: the target
    const TecmCombineOperand& op = o == c->M ? c->target : c->member[o];
    if (lds_h && op.stride_h == 1 && op.stride_i == c->H) {
      lds_mask |= 1 << (o == c->M ? mb : o);
      ++staged;
    }
  }
  const size_t lds = (size_t)staged * cmb_slab(mb) * sizeof(float);
  const dim3 grid((unsigned)tiles, (unsigned)chunks, (unsigned)c->G);
  switch (mb) {
    case 1: hipLaunchKernelGGL(combine_moments_kernel<1>, grid, dim3(256), lds, (hipStream_t)stream, *c, lds_mask); break;
    case 2: hipLaunchKernelGGL(combine_moments_kernel<2>, grid, dim3(256), lds, (hipStream_t)stream, *c, lds_mask); break;
    case 4: hipLaunchKernelGGL(combine_moments_kernel<4>, grid, dim3(256), lds, (hipStream_t)stream, *c, lds_mask); break;
    default: hipLaunchKernelGGL(combine_moments_kernel<8>, grid, dim3(256), lds, (hipStream_t)stream, *c, lds_mask); break;
  }
  TECM_CHECK_LAUNCH("tecm_combine_moments");
  return TECM_OK;
}

extern "C" int tecm_combine_solve(const TecmCombineSolve* c, void* stream) {
  TECM_REQUIRE(c, TECM_E_ARG, "tecm_combine_solve: null descriptor");
  TECM_REQUIRE(c->M >= 1 && c->M <= CMB_MAX, TECM_E_ARG, "tecm_combine_solve: M must be in [1, %d], got %d", CMB_MAX, c->M);
  TECM_REQUIRE(c->stats && c->weight && c->intercept && c->status && c->dropped, TECM_E_ARG, "tecm_combine_solve: null pointer");
  TECM_REQUIRE(c->G > 0 && c->H > 0 && c->I > 0, TECM_E_ARG, "tecm_combine_solve: bad shape");
  TECM_REQUIRE(c->ridge >= 0.0 && c->ridge <= 1.79769313486231570815e308, TECM_E_ARG,
               "tecm_combine_solve: ridge must be finite and >= 0");
  for (int m = 0; m < c->M; ++m)
    TECM_REQUIRE(c->w0[m] == c->w0[m] && fabs(c->w0[m]) <= 1.79769313486231570815e308, TECM_E_ARG,
                 "tecm_combine_solve: the prior must be finite (member %d)", m);
  TECM_REQUIRE(c->I <= INT64_MAX / (int64_t)sizeof(double) / CMB_MAX / c->H / c->G, TECM_E_ARG,
               "tecm_combine_solve: G * H * M * I doubles do not fit 64-bit addressing");
  const int64_t cells = (int64_t)c->G * c->H * c->I, blocks = (cells + 255) / 256;
  TECM_REQUIRE(blocks <= 2147483647LL, TECM_E_ARG, "tecm_combine_solve: more than 2^31 - 1 blocks of 256 cells");
  TECM_REQUIRE(tecm_aligned(c->stats, 8) && tecm_aligned(c->weight, 8) && tecm_aligned(c->intercept, 8) &&
               tecm_aligned(c->status, 4), TECM_E_ALIGN,
               "tecm_combine_solve: stats, weight and intercept must be 8-byte aligned, status 4-byte aligned");
  const dim3 grid((unsigned)blocks);
  switch (cmb_bucket(c->M)) {
    case 1: hipLaunchKernelGGL(combine_solve_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, *c); break;
    case 2: hipLaunchKernelGGL(combine_solve_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, *c); break;
    case 4: hipLaunchKernelGGL(combine_solve_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, *c); break;
    default: hipLaunchKernelGGL(combine_solve_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, *c); break;
  }
  TECM_CHECK_LAUNCH("tecm_combine_solve");
  return TECM_OK;
}

extern "C" int tecm_combine_apply(const TecmCombineApply* c, void* stream) {
  TECM_REQUIRE(c, TECM_E_ARG, "tecm_combine_apply: null descriptor");
  TECM_REQUIRE(c->M >= 1 && c->M <= CMB_MAX, TECM_E_ARG, "tecm_combine_apply: M must be in [1, %d], got %d", CMB_MAX, c->M);
  for (int m = 0; m < c->M; ++m)
    TECM_REQUIRE(c->member[m].base, TECM_E_ARG, "tecm_combine_apply: null pointer (member %d)", m);
  TECM_REQUIRE(c->weight && c->intercept && c->out && c->err_flag, TECM_E_ARG, "tecm_combine_apply: null pointer");
  TECM_REQUIRE(c->S > 0 && c->H > 0 && c->I > 0 && c->G > 0, TECM_E_ARG, "tecm_combine_apply: bad shape");
  const int64_t chunks = ((int64_t)c->H + CMB_HC - 1) / CMB_HC, tiles = (c->I + CMB_TILE - 1) / CMB_TILE;
  TECM_REQUIRE(chunks <= 65535, TECM_E_ARG, "tecm_combine_apply: ceil(H / 4) must be <= 65535");
  TECM_REQUIRE(tiles <= 2147483647LL, TECM_E_ARG, "tecm_combine_apply: more than 2^31 - 1 tiles of 64 nodes");
  TECM_REQUIRE(tecm_aligned(c->weight, 8) && tecm_aligned(c->intercept, 8) && tecm_aligned(c->out, 4) &&
               tecm_aligned(c->group, 4) && tecm_aligned(c->err_flag, 4), TECM_E_ALIGN,
               "tecm_combine_apply: weight and intercept must be 8-byte aligned, out, group and err_flag 4-byte aligned");
  const int64_t zs = c->S < 65535 ? c->S : 65535;
  hipLaunchKernelGGL(combine_apply_kernel, dim3((unsigned)tiles, (unsigned)chunks, (unsigned)zs), dim3(256), 0,
                     (hipStream_t)stream, *c);
  TECM_CHECK_LAUNCH("tecm_combine_apply");
  return TECM_OK;
}
