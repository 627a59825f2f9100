// Gradient of the fused stage a-1..a-3 with respect to its INPUT x (the forward: spatial_fwd.hip / spatial_fwd2.hip; the
// parameter gradients: spatial_bwd.hip / spatial_bwd2.hip, which form d x_l per tile from the tile's own edges only and so
// cannot store d x).  Per graph g = (b, t), rows h_n = [x_n | node_emb_n + temb], x_l = W_l h + b_l, x_r = W_r h + b_r,
// e_ij = att_k . lrelu(x_l[j,k] + x_r[i,k]), alpha = softmax over the in-edges of i plus its self loop, alpha~ = alpha * mult
// (the forward's alpha dropout), out_i = h_i + sum_j alpha~_ij x_l[j] + bias.  Given dout:
//     dalpha_ij = mult_ij <dout_i[k], x_l[j,k]>          de_ij = alpha_ij (dalpha_ij - sum_j' alpha_ij' dalpha_ij')
//     d x_l[j,k] += alpha~_ij dout_i[k] + de_ij att_k (.) lrelu'(s)          d x_r[i,k] += de_ij att_k (.) lrelu'(s)
//     dx_n = dout_n[:Cin] + W_l[:, :Cin]^T d x_l[n] + W_r[:, :Cin]^T d x_r[n]
// Three launches per chunk of graphs, no float atomics, every sum in a fixed order -- dx is bit-reproducible:
//   rows    thread = (row, transform): x_l and x_r of every row of the chunk -> workspace (24-float rows, one head per
//           12-float half).  Nothing is tiled, so no window limits apply and per-node time features cost nothing extra; a
//           time index outside its table gives a NaN row and sets the error word, as in the forward.
//   target  thread = (target i, head): two sweeps over the in-edges of i (by-target CSR) with online-softmax statistics;
//           writes (running max, 1 / denominator, sum alpha dalpha) per (i, head) for the source side, forms d x_r[i] and
//           stores dx_i = dout_i[:Cin] + W_r[:, :Cin]^T d x_r[i] (the two heads of a row sit in neighbouring lanes).
//   source  thread = (source j, head): sweeps the out-edges of j (whole-graph by-source CSR; every entry carries its target
//           and its slot in the target's list, so the dropout index is the forward's), recomputes e, alpha, mult and de from
//           the statistics, sums d x_l[j] and adds W_l[:, :Cin]^T d x_l[j] to dx_j -- one writer per row.
// In a graph without edges (graphs_with_edges) only the self loop is swept, at slot 0: alpha = 1, de = 0.
// The logit, the online-softmax step, the de accumulations and the dropout mask index are spatial_edge.h's; the rows kernel
// is restated in spatial_attn.hip (see there for why the two do not share one body).
// The workspace holds one chunk of graphs (<= 64 MiB), the launcher walks the chunks.
#include <cstdlib>
#include "spatial_edge.h"

using namespace tecm_spatial;

namespace {

constexpr int SW = 8;                   // statistics per row: per head (max, 1 / denominator, sum alpha dalpha, pad)
constexpr int WS_ROW = 2 * CP + SW;     // workspace floats per row: x_l | x_r | statistics

struct DxArgs {
  TecmSpatial d;
  TecmSpatialDx g;
  int g0, gc;                           // graphs [g0, g0 + gc) in memory order gm = b*L + t
};

// what a (row, head) thread of the target / source kernels knows about itself
struct RowId {
  int r, hh, node, rowbase;             // row inside the chunk (clamped), head, node id, chunk row of node 0 of the graph
  int64_t grow;                         // row of node 0 of the graph in the (B, L, N, *) tensors
  int64_t mrow;                         // ... and in the reference's (L*B, N) flattening (dropout index)
  bool on, use_edges;
};
__device__ __forceinline__ RowId row_id(const DxArgs& a) {
  const TecmSpatial& d = a.d;
  const int rows = a.gc * d.N;
  const int idx = blockIdx.x * TB + threadIdx.x;
  RowId q;
  q.hh = idx & 1;
  q.on = (idx >> 1) < rows;
  q.r = min(idx >> 1, rows - 1);
  const int gl = q.r / d.N, gm = a.g0 + gl;
  q.node = q.r - gl * d.N;
  q.rowbase = gl * d.N;
  const Graph g = decode_graph(d, gm);
  q.grow = (int64_t)gm * d.N;
  q.mrow = (int64_t)(g.t * d.B + g.b) * d.N;
  q.use_edges = g.use_edges;
  return q;
}

// ---- rows: x_l (blockIdx.y == 0) or x_r (1) of 256 rows of the chunk
template <int CIN>
__global__ __launch_bounds__(TB) void spatial_dx_rows_kernel(const DxArgs a) {
  constexpr int DEMB = C - CIN;
  __shared__ __attribute__((aligned(16))) float sW[C * CP];
  const TecmSpatial& d = a.d;
  const int m = blockIdx.y, tid = threadIdx.x;
  const float* __restrict__ W = m ? d.Wr : d.Wl;
  const float* __restrict__ bv = m ? d.br : d.bl;
  for (int k = tid; k < C * CP; k += TB) {
    const int ch = k / CP, kk = k - ch * CP;
    sW[k] = kk < C ? W[ch * C + kk] : 0.f;
  }
  __syncthreads();
  const int rows = a.gc * d.N;
  const int r = blockIdx.x * TB + tid;
  if (r >= rows) return;
  const int gl = r / d.N, node = r - gl * d.N, gm = a.g0 + gl;
  const Graph g = decode_graph(d, gm);
  float h[CP];
  const float2* xp = reinterpret_cast<const float2*>(d.x + ((int64_t)gm * d.N + node) * CIN);
#pragma unroll
  for (int k = 0; k < CIN / 2; ++k) {
    const float2 v = xp[k];
    h[2 * k] = v.x;
    h[2 * k + 1] = v.y;
  }
  const TimeIdx ti = load_time_idx(d, g.b, g.t, node);
#pragma unroll
  for (int e = 0; e < DEMB; ++e) h[CIN + e] = d.node_tab[(int64_t)node * DEMB + e] + temporal_emb(d, ti, e);
  h[C] = h[C + 1] = 0.f;
  float o[CP];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const float4* w4 = reinterpret_cast<const float4*>(sW + ch * CP);
    float v = bv[ch];
#pragma unroll
    for (int q = 0; q < CP / 4; ++q) {
      const float4 w = w4[q];
      v = fmaf(w.x, h[4 * q], v);
      v = fmaf(w.y, h[4 * q + 1], v);
      v = fmaf(w.z, h[4 * q + 2], v);
      v = fmaf(w.w, h[4 * q + 3], v);
    }
    o[slot_of(ch)] = v;
  }
  o[CH] = o[2 * CH + 1] = 0.f;
  float4* dst = reinterpret_cast<float4*>(a.g.ws + ((int64_t)m * rows + r) * CP);
#pragma unroll
  for (int q = 0; q < CP / 4; ++q) dst[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
}

// W_m[:, :Cin]^T of this head's d x_m, both heads summed (the partner head is the neighbouring lane)
template <int CIN>
__device__ __forceinline__ void to_input(const float* sWm, int hh, const float (&dxm)[CH], float (&tot)[CIN]) {
#pragma unroll
  for (int k = 0; k < CIN; ++k) {
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) v = fmaf(sWm[(hh * CH + c) * CIN + k], dxm[c], v);
    tot[k] = v + __shfl_xor(v, 1);
  }
}
template <int CIN>
__device__ __forceinline__ void stage_input_cols(const float* __restrict__ W, float* sWm) {
  for (int k = threadIdx.x; k < C * CIN; k += TB) {
    const int ch = k / CIN;
    sWm[k] = W[ch * C + (k - ch * CIN)];
  }
  __syncthreads();
}

// ---- target: thread = (target row, head)
template <int CIN>
__global__ __launch_bounds__(TB) void spatial_dx_target_kernel(const DxArgs a) {
  __shared__ float sWr[C * CIN];
  const TecmSpatial& d = a.d;
  stage_input_cols<CIN>(d.Wr, sWr);
  const RowId q = row_id(a);
  const int rows = a.gc * d.N, i = q.node, hh = q.hh;
  const float* __restrict__ XL = a.g.ws;
  const float* __restrict__ XR = a.g.ws + (int64_t)rows * CP;
  float* __restrict__ ST = a.g.ws + (int64_t)2 * rows * CP;
  float xr[CH + 1], gv[CH], att[CH], dxr[CH];
  ld12(XR + (int64_t)q.r * CP + hh * HP, xr);
  const float* gp = a.g.dout + (q.grow + i) * CP + hh * CH;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    gv[c] = gp[c];
    att[c] = d.att[hh * CH + c];
    dxr[c] = 0.f;
  }
  const AlphaDrop dr = alpha_drop_of(d);
  const uint64_t dseed = alpha_drop_seed(d);
  const uint64_t dbase = alpha_drop_base(d, q.mrow + i, hh);
  const int e0 = d.rowptr[i];
  const int deg = q.use_edges ? d.rowptr[i + 1] - e0 : 0;
  const float* xlg = XL + (int64_t)q.rowbase * CP + hh * HP;
  // sweep 1: logits and dalpha, online-softmax statistics; slot deg is the implicit self loop
  float mx = -INFINITY, z = 0.f, num = 0.f;
  for (int s = 0; s <= deg; ++s) {
    const int j = s < deg ? d.colidx[e0 + s] : i;
    float al[CH + 1];
    ld12(xlg + (int64_t)j * CP, al);
    const float e = logit_lrelu(al, xr, att);
    float da = dot11(gv, al);
    if (dr.th) da *= alpha_drop_mult(dr, dseed, dbase + s);
    softmax_step(e, da, LOG2E, mx, z, num);
  }
  const float zinv = 1.0f / (z + 1e-16f);
  const float dot = num * zinv;
  // sweep 2: de per edge, d x_r
  for (int s = 0; s <= deg; ++s) {
    const int j = s < deg ? d.colidx[e0 + s] : i;
    float al[CH + 1];
    ld12(xlg + (int64_t)j * CP, al);
    const float e = logit_lrelu(al, xr, att);
    float da = dot11(gv, al);
    if (dr.th) da *= alpha_drop_mult(dr, dseed, dbase + s);
    de_to_dxr(__builtin_amdgcn_exp2f((e - mx) * LOG2E) * zinv * (da - dot), al, xr, att, dxr);
  }
  float tot[CIN];
  to_input<CIN>(sWr, hh, dxr, tot);
  if (!q.on) return;
  *reinterpret_cast<float4*>(ST + ((int64_t)q.r * 2 + hh) * 4) = make_float4(mx, zinv, dot, 0.f);
  if (hh == 0) {
    const float* g0p = a.g.dout + (q.grow + i) * CP;
    float* dxp = a.g.dx + (q.grow + i) * a.g.dx_ld;
#pragma unroll
    for (int k = 0; k < CIN; ++k) dxp[k] = g0p[k] + tot[k];
  }
}

// ---- source: thread = (source row, head)
template <int CIN>
__global__ __launch_bounds__(TB) void spatial_dx_source_kernel(const DxArgs a) {
  __shared__ float sWl[C * CIN];
  const TecmSpatial& d = a.d;
  stage_input_cols<CIN>(d.Wl, sWl);
  const RowId q = row_id(a);
  const int rows = a.gc * d.N, j = q.node, hh = q.hh;
  const float* __restrict__ XL = a.g.ws;
  const float* __restrict__ XR = a.g.ws + (int64_t)rows * CP;
  const float* __restrict__ ST = a.g.ws + (int64_t)2 * rows * CP;
  float xl[CH + 1], att[CH], dxl[CH];
  ld12(XL + (int64_t)q.r * CP + hh * HP, xl);
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    att[c] = d.att[hh * CH + c];
    dxl[c] = 0.f;
  }
  const AlphaDrop dr = alpha_drop_of(d);
  const uint64_t dseed = alpha_drop_seed(d);
  const int q0 = q.use_edges ? a.g.src_rowptr[j] : 0, q1 = q.use_edges ? a.g.src_rowptr[j + 1] : 0;
  const int self_slot = q.use_edges ? d.rowptr[j + 1] - d.rowptr[j] : 0;
  for (int p = q0; p <= q1; ++p) {                            // the out-edges of j in list order, then its self loop
    const int i = p < q1 ? a.g.src_target[p] : j;
    const int slot = p < q1 ? a.g.src_slot[p] : self_slot;
    float xr[CH + 1], gt[CH];
    ld12(XR + (int64_t)(q.rowbase + i) * CP + hh * HP, xr);
    const float* gp = a.g.dout + (q.grow + i) * CP + hh * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) gt[c] = gp[c];
    const float4 st = *reinterpret_cast<const float4*>(ST + ((int64_t)(q.rowbase + i) * 2 + hh) * 4);
    const float e = logit_lrelu(xl, xr, att);
    float mult = 1.0f;
    if (dr.th) mult = alpha_drop_mult(dr, dseed, alpha_drop_base(d, q.mrow + i, hh) + slot);
    const float alpha = __builtin_amdgcn_exp2f((e - st.x) * LOG2E) * st.y;
    const float de = alpha * (dot11(gt, xl) * mult - st.z);
    de_to_dxl(alpha * mult, de, gt, xl, xr, att, dxl);
  }
  float tot[CIN];
  to_input<CIN>(sWl, hh, dxl, tot);
  if (!q.on || hh != 0) return;
  float* dxp = a.g.dx + (q.grow + j) * a.g.dx_ld;
#pragma unroll
  for (int k = 0; k < CIN; ++k) dxp[k] += tot[k];
}

bool served(const TecmSpatial& d) { return d.flags == 0 && (d.Cin == 10 || d.Cin == 6) && d.Demb == C - d.Cin; }

// graphs per chunk: what fits WS_CHUNK_BYTES, at least one
int chunk_graphs(const TecmSpatial& d) {
  int64_t gc = WS_CHUNK_BYTES / ((int64_t)d.N * WS_ROW * (int64_t)sizeof(float));
  if (const char* e = std::getenv("TECM_SPATIAL_DX_GRAPHS")) {   // diagnostics: graphs per chunk
    const int v = atoi(e);
    if (v > 0) gc = v;
  }
  const int64_t G = (int64_t)d.B * d.L;
  return (int)(gc < 1 ? 1 : (gc > G ? G : gc));
}

template <int CIN>
int launch_chunks(const TecmSpatial& d, const TecmSpatialDx& g, hipStream_t st) {
  const int G = d.B * d.L, gcmax = chunk_graphs(d);
  for (int g0 = 0; g0 < G; g0 += gcmax) {
    DxArgs a;
    a.d = d;
    a.g = g;
    a.g0 = g0;
    a.gc = G - g0 < gcmax ? G - g0 : gcmax;
    const int64_t rows = (int64_t)a.gc * d.N;
    hipLaunchKernelGGL(spatial_dx_rows_kernel<CIN>, dim3((unsigned)((rows + TB - 1) / TB), 2), dim3(TB), 0, st, a);
    TECM_CHECK_LAUNCH("tecm_spatial_dx(rows)");
    const dim3 grid((unsigned)((2 * rows + TB - 1) / TB));
    hipLaunchKernelGGL(spatial_dx_target_kernel<CIN>, grid, dim3(TB), 0, st, a);
    TECM_CHECK_LAUNCH("tecm_spatial_dx(target)");
    hipLaunchKernelGGL(spatial_dx_source_kernel<CIN>, grid, dim3(TB), 0, st, a);
    TECM_CHECK_LAUNCH("tecm_spatial_dx(source)");
  }
  return TECM_OK;
}

}  // namespace

// Floats of workspace tecm_spatial_dx needs for `d`, or 0 when it does not serve the call.
extern "C" int64_t tecm_spatial_dx_ws_floats(const TecmSpatial* dp) {
  if (dp == nullptr || check_common("tecm_spatial_dx_ws_floats", *dp) != TECM_OK || !served(*dp)) return 0;
  if ((int64_t)dp->N * chunk_graphs(*dp) >= (int64_t)1 << 29) return 0;   // chunk rows are 32-bit (two threads per row)
  return (int64_t)chunk_graphs(*dp) * dp->N * WS_ROW;
}

extern "C" int tecm_spatial_dx(const TecmSpatial* dp, const TecmSpatialDx* gp, void* stream) {
  TECM_REQUIRE(dp != nullptr && gp != nullptr, TECM_E_ARG, "tecm_spatial_dx: null descriptor");
  const TecmSpatial& d = *dp;
  const TecmSpatialDx& g = *gp;
  const int rc = check_common("tecm_spatial_dx", d);
  if (rc) return rc;
  TECM_REQUIRE(served(d), TECM_E_ARG,
               "tecm_spatial_dx: serves the fused stage (flags = 0) with Cin 6 or 10 and Demb = 22 - Cin (got flags=%d Cin=%d Demb=%d)",
               d.flags, d.Cin, d.Demb);
  TECM_REQUIRE(tecm_spatial_dx_ws_floats(dp) > 0, TECM_E_ARG, "tecm_spatial_dx: too many rows per graph");
  TECM_REQUIRE(g.dout && g.dx && g.ws && g.src_rowptr && g.src_target && g.src_slot, TECM_E_ARG, "tecm_spatial_dx: null pointer");
  TECM_REQUIRE(g.dx_ld >= d.Cin, TECM_E_ARG, "tecm_spatial_dx: dx_ld must be >= Cin");
  TECM_REQUIRE(tecm_aligned(g.dout, 16) && tecm_aligned(g.ws, 16) && tecm_aligned(d.x, 8), TECM_E_ALIGN,
               "tecm_spatial_dx: dout and the workspace must be 16-byte aligned, x 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  return d.Cin == 10 ? launch_chunks<10>(d, g, st) : launch_chunks<6>(d, g, st);
}
