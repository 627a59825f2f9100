// Causal multi-head attention for 33 <= T <= 1024 tokens per (b, n) sequence, head_dim 64 -- the long-window routes of
// tecm_attention_fwd / tecm_attention_bwd (attention.hip keeps T <= 32).  Same contract as those kernels: time-major rows
// (token p of sequence (b, n) is row (b*T + p)*N + n of the (B,T,N,3D) qkv buffer), scale 1/8, row i attends to j <= i,
// dropout on the probabilities with idx = (((b*N + n)*H + h)*T + i)*T + j (64-bit) and the seed of tecm_seed_now.
//
// Every product runs on v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain) over 16 x 16 tiles; scores,
// softmax, probabilities, dP and dS stay fp32 and bf16 appears only at the io_bf16 loads / stores.  Lane l of a wave has
// r16 = l & 15 and g = l >> 4; the MFMA takes A[r16][g], B[g][r16] per lane and returns C[4g + r][r16] in register r.
//  - "row fragment" of a 16-row block: lane l holds row r16, dims 16g .. 16g+15 (four float4), so a 64-dim dot product of
//    two row blocks is 16 MFMAs (k-step s pairs dim 16g + s of both operands);
//  - such a tile with KEYS on its rows (S^T = K Q^T: key 4g + r in register r, query r16 on the lane) is directly the B
//    operand of a product that sums over keys (k-step r = key 4g + r); its A operand is the "step fragment" of the other
//    matrix: lane l holds row 4g + r, dims 4*r16 .. 4*r16+3 for r = 0..3, so output row 4g + r' of MFMA db is dim
//    16g + 4r' + db and each lane ends with dims 16g .. 16g+15 of one row: four float4 stores.
// Forward: one wave per (sequence, head, 16-query block), online softmax over the 16-key tiles up to the diagonal.
// Backward: one workgroup per (sequence, head) and no workspace: (1) per query row, the softmax statistics m, 1/l and
// delta = sum_j P_ij dP_ij into LDS; (2) per 16-key block, dK and dV over the query blocks at or below it (key-major, no
// sum across waves); (3) per query block, dQ over the key tiles (query-major).  P and dP are recomputed in each pass.
// No atomics, no scratch (SPILL_CEILINGS in __graft_entry__.py), bit-identical from launch to launch.
#include "attention_long.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct DropL {
  uint64_t seed;
  uint32_t thresh;
  float inv;
  const uint64_t* sdev;        // TecmDrop::seed_dev: added to seed when the kernel starts
};

constexpr float kScale = 0.125f;  // 1/sqrt(64)

// four consecutive elements at element offset `off` of an fp32 or (B16) bf16 tensor, as floats
template <bool B16>
__device__ __forceinline__ f32x4 ld4(const float* __restrict__ p, int64_t off) {
  if constexpr (B16) {
    const tecm_bf16x4 h = *reinterpret_cast<const tecm_bf16x4*>(reinterpret_cast<const __bf16*>(p) + off);
    return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
  } else {
    return *reinterpret_cast<const f32x4*>(p + off);
  }
}

__device__ __forceinline__ void st4(float* p, int bf16, int64_t off, f32x4 v) {
  if (bf16)
    tecm_store_bf16x4(reinterpret_cast<__bf16*>(p) + off, v[0], v[1], v[2], v[3]);
  else
    *reinterpret_cast<f32x4*>(p + off) = v;
}

// Addressing of one (sequence, head): token p's element c of column block `part` (0 q, 1 k, 2 v / the dctx row) is at
// (row0 + p*N) * ld + col + c.  Rows at or past T are never read: they come back as zeros.
struct Seq {
  int64_t row0, N;
  int T;
  __device__ __forceinline__ int64_t at(int p, int64_t ld, int col) const { return (row0 + (int64_t)p * N) * ld + col; }
};

// row fragment: lane holds row `p`, dims 16g .. 16g+15 of the 64 starting at column `col`
template <bool B16>
__device__ __forceinline__ void load_rows(f32x4 (&f)[4], const float* __restrict__ base, const Seq& s, int64_t ld,
                                          int col, int p, int g) {
#pragma unroll
  for (int c = 0; c < 4; ++c) f[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (p < s.T) {
#pragma unroll
    for (int c = 0; c < 4; ++c) f[c] = ld4<B16>(base, s.at(p, ld, col + 16 * g + 4 * c));
  }
}

// step fragment of the 16-row block starting at token p0: f[r] = row p0 + 4g + r, dims 4*r16 .. 4*r16+3
template <bool B16>
__device__ __forceinline__ void load_steps(f32x4 (&f)[4], const float* __restrict__ base, const Seq& s, int64_t ld,
                                           int col, int p0, int g, int r16) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int p = p0 + 4 * g + r;
    f[r] = p < s.T ? ld4<B16>(base, s.at(p, ld, col + 4 * r16)) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// C[4g + r][r16] = sum over the 64 dims of A-row r16 . B-row r16 (both row fragments)
__device__ __forceinline__ f32x4 dot_rows(const f32x4 (&a)[4], const f32x4 (&b)[4]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][e], b[c][e], acc, 0, 0, 0);
  return acc;
}

// acc[db] += step fragment (as A: row 4*r16 + db, k = 4g + r)  x  tile (as B: register r = row 4g + r, column r16)
__device__ __forceinline__ void acc_steps(f32x4 (&acc)[4], const f32x4 (&a)[4], const float (&t)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int db = 0; db < 4; ++db) acc[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r][db], t[r], acc[db], 0, 0, 0);
}

// lane's dims 16g .. 16g+15 of the accumulators of acc_steps, times `mul`, to row offset `off`
__device__ __forceinline__ void store_acc(float* p, int bf16, int64_t off, const f32x4 (&acc)[4], float mul, int g) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    st4(p, bf16, off + 16 * g + 4 * r, f32x4{acc[0][r] * mul, acc[1][r] * mul, acc[2][r] * mul, acc[3][r] * mul});
}

// over the four 16-lane groups (the tile rows 4g + r that register r does not cover)
__device__ __forceinline__ float groups_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float groups_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

__device__ __forceinline__ float drop_mult(const DropL& dr, int64_t sh, int T, int i, int j) {
  return tecm_drop_mult(dr.seed, (uint64_t)((sh * T + i) * T + j), dr.thresh, dr.inv);
}

// ------------------------------------------------------------------ forward
// One wave per (sequence, head, 16-query block); the heaviest block of a (sequence, head) goes first.
template <bool Q16>
__global__ __launch_bounds__(256) void att_long_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ ctx,
                                                           int ctx_bf16, int B, int T, int N, int H, DropL dr) {
  dr.seed = tecm_seed_now(dr.seed, dr.sdev);
  const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
  const int QB = (T + 15) >> 4;
  const int64_t item = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (item >= (int64_t)B * N * H * QB) return;    // whole waves leave together
  const int64_t sh = item / QB;                   // (b*N + n)*H + h
  const int qb = QB - 1 - (int)(item - sh * QB);
  const int64_t seq = sh / H;
  const int h = (int)(sh - seq * H);
  const int b = (int)(seq / N), n = (int)(seq - (int64_t)b * N);
  const int D = H * 64;
  const int64_t ld = 3 * (int64_t)D;
  const Seq s{(int64_t)b * T * N + n, N, T};
  const int i = qb * 16 + r16;                    // this lane's query: the column of every tile

  f32x4 qf[4], kf[4], vs[4];
  load_rows<Q16>(qf, qkv, s, ld, h * 64, i, g);
  load_rows<Q16>(kf, qkv, s, ld, D + h * 64, r16, g);
  load_steps<Q16>(vs, qkv, s, ld, 2 * D + h * 64, 0, g, r16);
  f32x4 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  for (int kt = 0; kt <= qb; ++kt) {
    const f32x4 st = dot_rows(kf, qf);            // S^T: register r = key kt*16 + 4g + r
    f32x4 vcur[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) vcur[r] = vs[r];
    if (kt < qb) {                                // the next tile's loads fly under this tile's softmax and P.V
      load_rows<Q16>(kf, qkv, s, ld, D + h * 64, (kt + 1) * 16 + r16, g);
      load_steps<Q16>(vs, qkv, s, ld, 2 * D + h * 64, (kt + 1) * 16, g, r16);
    }
    float sc[4], tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sc[r] = kt * 16 + 4 * g + r <= i ? st[r] * kScale : -INFINITY;
      tmax = fmaxf(tmax, sc[r]);
    }
    const float mn = fmaxf(m, groups_max(tmax));  // finite: key kt*16 <= i for every lane
    const float alpha = expf(m - mn);
    float p[4], ts = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[r] = expf(sc[r] - mn);
      ts += p[r];
      if (dr.thresh && i < T && kt * 16 + 4 * g + r <= i) p[r] *= drop_mult(dr, sh, T, i, kt * 16 + 4 * g + r);
    }
    l = l * alpha + groups_sum(ts);
    m = mn;
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] *= alpha;
    acc_steps(o, vcur, p);
  }
  if (i < T) store_acc(ctx, ctx_bf16, s.at(i, D, h * 64), o, 1.0f / l, g);
}

// ------------------------------------------------------------------ backward
// One workgroup of min(4, QB) waves per (sequence, head).  LDS: m (of the scaled scores), 1/l and delta per query row.
__device__ __forceinline__ int snake(int t, int w, int nw) { return t * nw + ((t & 1) ? nw - 1 - w : w); }

template <bool Q16, bool D16>
__global__ __launch_bounds__(256) void att_long_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                           float* __restrict__ dqkv, int dqkv_bf16, int T, int N, int H,
                                                           DropL dr) {
  extern __shared__ float lds[];                  // [3][16*QB]
  dr.seed = tecm_seed_now(dr.seed, dr.sdev);
  const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int QB = (T + 15) >> 4, TP = QB * 16;
  float* st_m = lds;
  float* st_il = lds + TP;
  float* st_dl = lds + 2 * TP;
  const int64_t sh = blockIdx.x;                  // (b*N + n)*H + h
  const int64_t seq = sh / H;
  const int h = (int)(sh - seq * H);
  const int b = (int)(seq / N), n = (int)(seq - (int64_t)b * N);
  const int D = H * 64;
  const int64_t ld = 3 * (int64_t)D;
  const Seq s{(int64_t)b * T * N + n, N, T};
  const int cq = h * 64, ck = D + h * 64, cv = 2 * D + h * 64;

  // (1) statistics of every query row: m = max_j s_ij, l = sum_j exp(s_ij - m), delta = sum_j P_ij dP_ij
  for (int t = 0;; ++t) {
    const int qb = snake(t, w, nw);
    if (qb >= QB) break;
    const int i = qb * 16 + r16;
    f32x4 qf[4], of[4];
    load_rows<Q16>(qf, qkv, s, ld, cq, i, g);
    load_rows<D16>(of, dctx, s, D, h * 64, i, g);
    float m = -INFINITY, l = 0.f, dl = 0.f;
    for (int kt = 0; kt <= qb; ++kt) {
      f32x4 kf[4], vf[4];
      load_rows<Q16>(kf, qkv, s, ld, ck, kt * 16 + r16, g);
      load_rows<Q16>(vf, qkv, s, ld, cv, kt * 16 + r16, g);
      const f32x4 st = dot_rows(kf, qf);          // S^T
      const f32x4 dpt = dot_rows(vf, of);         // dP~^T = V dctx^T
      float sc[4], tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sc[r] = kt * 16 + 4 * g + r <= i ? st[r] * kScale : -INFINITY;
        tmax = fmaxf(tmax, sc[r]);
      }
      const float mn = fmaxf(m, groups_max(tmax));
      const float alpha = expf(m - mn);
      float ts = 0.f, td = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = expf(sc[r] - mn);
        float dp = dpt[r];
        if (dr.thresh && i < T && kt * 16 + 4 * g + r <= i) dp *= drop_mult(dr, sh, T, i, kt * 16 + 4 * g + r);
        ts += p;
        td += p * dp;
      }
      l = l * alpha + groups_sum(ts);
      dl = dl * alpha + groups_sum(td);
      m = mn;
    }
    if (g == 0) {                                 // rows at or past T: P = 0 in passes 2 and 3
      st_m[i] = i < T ? m : 0.f;
      st_il[i] = i < T ? 1.0f / l : 0.f;
      st_dl[i] = i < T ? dl / l : 0.f;
    }
  }
  __syncthreads();

  // (2) dK, dV of key block kb: sums over the query blocks qb >= kb; tile C[query 4g + r][key r16]
  for (int kb = w; kb < QB; kb += nw) {
    const int j = kb * 16 + r16;
    f32x4 kf[4], vf[4], dk[4], dv[4];
    load_rows<Q16>(kf, qkv, s, ld, ck, j, g);
    load_rows<Q16>(vf, qkv, s, ld, cv, j, g);
#pragma unroll
    for (int db = 0; db < 4; ++db) dk[db] = dv[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int qb = kb; qb < QB; ++qb) {
      f32x4 qf[4], of[4], qs[4], os[4];
      load_rows<Q16>(qf, qkv, s, ld, cq, qb * 16 + r16, g);
      load_rows<D16>(of, dctx, s, D, h * 64, qb * 16 + r16, g);
      load_steps<Q16>(qs, qkv, s, ld, cq, qb * 16, g, r16);
      load_steps<D16>(os, dctx, s, D, h * 64, qb * 16, g, r16);
      const f32x4 sc = dot_rows(qf, kf);          // S
      const f32x4 dpt = dot_rows(of, vf);         // dP~ = dctx V^T
      float pt[4], ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int iq = qb * 16 + 4 * g + r;
        const bool ok = j <= iq && iq < T;
        const float p = ok ? expf(sc[r] * kScale - st_m[iq]) * st_il[iq] : 0.f;
        const float mu = dr.thresh && ok ? drop_mult(dr, sh, T, iq, j) : 1.0f;
        pt[r] = p * mu;
        ds[r] = p * (dpt[r] * mu - st_dl[iq]) * kScale;
      }
      acc_steps(dv, os, pt);                      // dV^T += dctx^T P~
      acc_steps(dk, qs, ds);                      // dK^T += Q^T dS
    }
    if (j < T) {
      store_acc(dqkv, dqkv_bf16, s.at(j, ld, ck), dk, 1.0f, g);
      store_acc(dqkv, dqkv_bf16, s.at(j, ld, cv), dv, 1.0f, g);
    }
  }

  // (3) dQ of query block qb: sum over the key tiles kt <= qb; tile C[key 4g + r][query r16]
  for (int qb = w; qb < QB; qb += nw) {
    const int i = qb * 16 + r16;
    const float m = st_m[i], il = st_il[i], dl = st_dl[i];
    f32x4 qf[4], of[4], dq[4];
    load_rows<Q16>(qf, qkv, s, ld, cq, i, g);
    load_rows<D16>(of, dctx, s, D, h * 64, i, g);
#pragma unroll
    for (int db = 0; db < 4; ++db) dq[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt <= qb; ++kt) {
      f32x4 kf[4], vf[4], ks[4];
      load_rows<Q16>(kf, qkv, s, ld, ck, kt * 16 + r16, g);
      load_rows<Q16>(vf, qkv, s, ld, cv, kt * 16 + r16, g);
      load_steps<Q16>(ks, qkv, s, ld, ck, kt * 16, g, r16);
      const f32x4 st = dot_rows(kf, qf);          // S^T
      const f32x4 dpt = dot_rows(vf, of);         // dP~^T
      float ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jk = kt * 16 + 4 * g + r;
        const bool ok = jk <= i && i < T;
        const float p = ok ? expf(st[r] * kScale - m) * il : 0.f;
        const float mu = dr.thresh && ok ? drop_mult(dr, sh, T, i, jk) : 1.0f;
        ds[r] = p * (dpt[r] * mu - dl) * kScale;
      }
      acc_steps(dq, ks, ds);                      // dQ^T += K^T dS^T
    }
    if (i < T) store_acc(dqkv, dqkv_bf16, s.at(i, ld, cq), dq, 1.0f, g);
  }
}

DropL make_dropl(const TecmDrop* d) {
  DropL r;
  r.seed = d ? d->seed : 0;
  r.sdev = d ? d->seed_dev : nullptr;
  r.thresh = (d && d->p > 0.f) ? tecm_drop_thresh(d->p) : 0u;
  r.inv = (d && d->p > 0.f) ? 1.0f / (1.0f - d->p) : 1.0f;
  return r;
}

}  // namespace

int att_long_fwd(const float* qkv, float* ctx, int32_t io_bf16, int32_t B, int32_t T, int32_t N, int32_t heads,
                 const TecmDrop* prob_drop, hipStream_t st) {
  const int ctx_bf16 = io_bf16 & TECM_ATT_OUT_BF16;
  const int64_t waves = (int64_t)B * N * heads * ((T + 15) / 16);
  TECM_REQUIRE((waves + 3) / 4 <= INT32_MAX, TECM_E_ARG, "tecm_attention_fwd: B*N*heads*ceil(T/16) too large");
  const dim3 grid((unsigned)((waves + 3) / 4));
  const DropL dr = make_dropl(prob_drop);
  if (io_bf16 & TECM_ATT_QKV_BF16)
    hipLaunchKernelGGL((att_long_fwd_kernel<true>), grid, dim3(256), 0, st, qkv, ctx, ctx_bf16, B, T, N, heads, dr);
  else
    hipLaunchKernelGGL((att_long_fwd_kernel<false>), grid, dim3(256), 0, st, qkv, ctx, ctx_bf16, B, T, N, heads, dr);
  TECM_CHECK_LAUNCH("tecm_attention_fwd");
  return TECM_OK;
}

int att_long_bwd(const float* qkv, const float* dctx, float* dqkv, int32_t io_bf16, int32_t B, int32_t T, int32_t N,
                 int32_t heads, const TecmDrop* prob_drop, hipStream_t st) {
  const int dqkv_bf16 = io_bf16 & TECM_ATT_OUT_BF16;
  const int64_t items = (int64_t)B * N * heads;
  TECM_REQUIRE(items <= INT32_MAX, TECM_E_ARG, "tecm_attention_bwd: B*N*heads too large");
  const int QB = (T + 15) / 16;
  const dim3 grid((unsigned)items), block(64 * (QB < 4 ? QB : 4));
  const size_t lds = 3 * sizeof(float) * 16 * QB;
  const DropL dr = make_dropl(prob_drop);
  const bool q16 = (io_bf16 & TECM_ATT_QKV_BF16) != 0, d16 = (io_bf16 & TECM_ATT_DCTX_BF16) != 0;
  if (q16 && d16)
    hipLaunchKernelGGL((att_long_bwd_kernel<true, true>), grid, block, lds, st, qkv, dctx, dqkv, dqkv_bf16, T, N, heads, dr);
  else if (q16)
    hipLaunchKernelGGL((att_long_bwd_kernel<true, false>), grid, block, lds, st, qkv, dctx, dqkv, dqkv_bf16, T, N, heads, dr);
  else
    hipLaunchKernelGGL((att_long_bwd_kernel<false, false>), grid, block, lds, st, qkv, dctx, dqkv, dqkv_bf16, T, N, heads, dr);
  TECM_CHECK_LAUNCH("tecm_attention_bwd");
  return TECM_OK;
}
