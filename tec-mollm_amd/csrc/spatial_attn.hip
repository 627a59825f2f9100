// The GATv2 attention coefficients of the fused stage a-1..a-3, handed to the caller (GATv2Conv modules.py:329-336,:356 with
// return_attention_weights=True; the forward: spatial_fwd.hip / spatial_fwd2.hip, which recompute them and keep none).
// Per graph (b, t), rows h_n = [x_n | node_emb_n + temb], x_l = W_l h + b_l, x_r = W_r h + b_r,
//     e_ij = att_k . lrelu(x_l[j,k] + x_r[i,k])        alpha_ij = exp(e_ij - max_j e_ij) / (sum_j exp(e_ij - max) + 1e-16)
// over the in-edges j of i plus its self loop: the coefficients BEFORE dropout (what eval() uses, what training draws its
// masks over).  With them, per (i, head) the entropy -sum_j alpha ln alpha and per entry the message size
// m_ij = alpha_ij * |x_l[j, head]|_2.
// Entry order inside a graph ("kernel order"): the by-target CSR entries q in [0, E') in rowptr / colidx order, then the N
// self loops at E' + i; E'' = E' + N.
// Three launches per chunk of graphs (memory order gm = b*L + t), no float atomics, every sum in a fixed order:
//   rows        thread = (row, transform): x_l and x_r of every row of the chunk -> workspace (24-float rows, one head per
//               12-float half); the pad float of each x_l half holds that head's L2 norm.  A time index outside its table
//               gives a NaN row and sets the error word, as in the forward.  Cin 6 / 10 (fused stage) or 22 (stand-alone
//               GATv2: the input rows are h, no table is read).
//   target      thread = (target i, head): sweep 1 gathers x_l[j], forms the logits, keeps their max and parks every logit in
//               the slot its coefficient will take; sweep 2 sums exp(e - max) over the parked logits; sweep 3 turns them
//               into alpha (and m, entropy).  The denominator is the sum of exactly the terms sweep 3 divides, so a row sums
//               to 1 within (deg + 2) * 2^-24 -- an online (rescaled) denominator would not give that bound -- and x_l is
//               gathered once, not twice.  In a graph without edges only the self loop exists: alpha = 1, every other
//               entry 0, entropy 0, all exact.  The raw export goes to alpha[(gm*E'' + p(q))*H + head] (p: optional
//               permutation of the CSR entries, so that the caller gets PyG's edge order in one pass).
//   accumulate  thread = (entry, head) or (node, head): walks the graphs of the chunk in ascending gm and adds alpha, alpha^2,
//               m (entropy) to the fp64 statistics of the graph's group with plain loads and stores -- one owner per cell,
//               so the same calls give the same bits, whatever the chunking.
// The workspace holds one chunk of graphs (<= 64 MiB unless one graph needs more), the launcher walks the chunks.
// The logit, the row loads and the graph decode are spatial_edge.h's, shared with the other spatial kernels.
#include "spatial_edge.h"

using namespace tecm_spatial;

namespace {

struct AttnArgs {
  TecmSpatial d;
  TecmSpatialAttn a;
  int g0, gc, gcap;                     // graphs [g0, g0 + gc) in memory order; gcap = graphs the workspace is laid out for
};

// workspace of a chunk laid out for gcap graphs: x_l rows | x_r rows | alpha | m | entropy (the last three only when the
// statistics are accumulated), alpha and m as (graph, entry, head), the entropy as (graph, node, head)
struct WsLayout {
  float *xl, *xr, *al, *ms, *en;
};
__host__ __device__ inline WsLayout ws_layout(const AttnArgs& q) {
  const int64_t rows = (int64_t)q.gcap * q.d.N, ent = (int64_t)q.gcap * ((int64_t)q.a.E + q.d.N) * H;
  WsLayout w;
  w.xl = q.a.ws;
  w.xr = w.xl + rows * CP;
  w.al = w.xr + rows * CP;
  w.ms = w.al + ent;
  w.en = w.ms + ent;
  return w;
}

// ---- rows: x_l (blockIdx.y == 0) or x_r (1) of 256 rows of the chunk.  spatial_dx_rows_kernel's transform plus the head
//      norms, restated here: as two entry points of one __device__ body (norms behind a template flag) the compiler packs
//      fewer of this kernel's FMAs (240 v_pk_fma_f32 + 48 v_fmac_f32 per row instead of 264 + 0) and the kernel measured
//      slower at B = 8, L = 48, N = 2911: <10> 194.7 -> 202.1 us per update (parent spread 0.3), spatial_dx_rows_kernel<10>
//      360.5 -> 364.5 us (spread 3.9); profiles/spatial_shared_math.txt.
template <int CIN>
__global__ __launch_bounds__(TB) void spatial_attn_rows_kernel(const AttnArgs a) {
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
  float h[CP];
  const float2* xp = reinterpret_cast<const float2*>(d.x + ((int64_t)gm * d.N + node) * CIN);
#pragma unroll
  for (int k = 0; k < CIN / 2; ++k) {
    const float2 v = xp[k];
    h[2 * k] = v.x;
    h[2 * k + 1] = v.y;
  }
  if constexpr (DEMB > 0) {
    const Graph g = decode_graph(d, gm);
    const TimeIdx ti = load_time_idx(d, g.b, g.t, node);
#pragma unroll
    for (int e = 0; e < DEMB; ++e) h[CIN + e] = d.node_tab[(int64_t)node * DEMB + e] + temporal_emb(d, ti, e);
  }
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
  // the two pad floats: |x_l[n, head]|_2 (the message size's factor), 0 in an x_r row
  float n0 = 0.f, n1 = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    n0 = fmaf(o[c], o[c], n0);
    n1 = fmaf(o[HP + c], o[HP + c], n1);
  }
  o[CH] = m ? 0.f : sqrtf(n0);
  o[2 * CH + 1] = m ? 0.f : sqrtf(n1);
  const WsLayout w = ws_layout(a);
  float4* dst = reinterpret_cast<float4*>((m ? w.xr : w.xl) + (int64_t)r * CP);
#pragma unroll
  for (int q = 0; q < CP / 4; ++q) dst[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
}

// ---- target: thread = (target row, head)
__global__ __launch_bounds__(TB) void spatial_attn_target_kernel(const AttnArgs a) {
  const TecmSpatial& d = a.d;
  const int rows = a.gc * d.N;
  const int idx = blockIdx.x * TB + threadIdx.x;
  if ((idx >> 1) >= rows) return;
  const int hh = idx & 1, r = idx >> 1;
  const int gl = r / d.N, i = r - gl * d.N, gm = a.g0 + gl;
  const bool use_edges = decode_graph(d, gm).use_edges;
  const int E1 = a.a.E, E2 = E1 + d.N;
  const bool acc = a.a.edge_stats != nullptr;
  const WsLayout w = ws_layout(a);
  float* wal = w.al + (int64_t)gl * E2 * H + hh;          // kernel order, chunk-local
  float* wms = w.ms + (int64_t)gl * E2 * H + hh;
  float* out = a.a.alpha ? a.a.alpha + (int64_t)gm * E2 * H + hh : nullptr;   // the caller's order
  const int32_t* __restrict__ perm = a.a.perm;
  const int e0 = d.rowptr[i], e1 = d.rowptr[i + 1];
  const int deg = use_edges ? e1 - e0 : 0;
  // slot s of this target: its s-th in-edge, slot deg the self loop.  entry(): kernel order; place(): where the raw export
  // puts it (a place outside [0, E'') is not written)
  auto entry = [&](int s) { return s < deg ? e0 + s : E1 + i; };
  auto place = [&](int q) { return (q < E1 && perm) ? perm[q] : q; };
  auto writable = [&](int p) { return (unsigned)p < (unsigned)E2; };
  if (!use_edges) {                                                   // the CSR entries of i exist in the layout: exact zeros
    for (int q = e0; q < e1; ++q) {
      if (acc) wal[(int64_t)q * H] = wms[(int64_t)q * H] = 0.f;
      const int p = place(q);
      if (out && writable(p)) out[(int64_t)p * H] = 0.f;
    }
  }
  float xr[CH + 1], att[CH];
  ld12(w.xr + (int64_t)r * CP + hh * HP, xr);
#pragma unroll
  for (int c = 0; c < CH; ++c) att[c] = d.att[hh * CH + c];
  const float* xlg = w.xl + (int64_t)gl * d.N * CP + hh * HP;
  // the logits are parked where the coefficients will go: the statistics' workspace, or else the caller's array
  float* park = acc ? wal : out;
  auto parked = [&](int q) { return (int64_t)(acc ? q : place(q)) * H; };
  // sweep 1: gather, logits, max
  float mx = -INFINITY;
  for (int s = 0; s <= deg; ++s) {
    const int j = s < deg ? d.colidx[e0 + s] : i, q = entry(s);
    float al[CH + 1];                                                 // al[CH]: the head's norm
    ld12(xlg + (int64_t)j * CP, al);
    const float e = logit_lrelu(al, xr, att);
    mx = fmaxf(mx, e);
    if (acc) wms[(int64_t)q * H] = al[CH];
    if (acc || writable(place(q))) park[parked(q)] = e;
  }
  // sweep 2: the denominator, from the terms sweep 3 divides
  float z = 0.f;
  for (int s = 0; s <= deg; ++s) {
    const int q = entry(s);
    if (acc || writable(place(q))) z += __builtin_amdgcn_exp2f((park[parked(q)] - mx) * LOG2E);
  }
  const float zinv = 1.0f / (z + 1e-16f);
  // sweep 3: alpha, message size, entropy (fp64: the accumulated statistic is compared against fp64 sums)
  double ent = 0.0;
  for (int s = 0; s <= deg; ++s) {
    const int q = entry(s), p = place(q);
    if (!acc && !writable(p)) continue;
    const float al = __builtin_amdgcn_exp2f((park[parked(q)] - mx) * LOG2E) * zinv;
    if (out && writable(p)) out[(int64_t)p * H] = al;
    if (acc) {
      wal[(int64_t)q * H] = al;
      wms[(int64_t)q * H] *= al;
      if (al != 0.f) ent -= (double)al * log((double)al);
    }
  }
  if (acc) w.en[((int64_t)gl * d.N + i) * H + hh] = (float)ent;
}

// ---- accumulate: thread = (entry, head) for the edge statistics, then (node, head) for the entropy; thread 0 also counts
__global__ __launch_bounds__(TB) void spatial_attn_accumulate_kernel(const AttnArgs a) {
  const TecmSpatial& d = a.d;
  const TecmSpatialAttn& s = a.a;
  const int64_t E2H = ((int64_t)s.E + d.N) * H, NH = (int64_t)d.N * H;
  const int64_t tid = (int64_t)blockIdx.x * TB + threadIdx.x;
  if (tid >= E2H + NH) return;
  const bool edge = tid < E2H;
  const int64_t cell = edge ? tid : tid - E2H;
  const WsLayout w = ws_layout(a);
  const bool skip = (s.flags & TECM_ATTN_SKIP_UNCONNECTED) != 0;
  int cur = -1;
  bool bad = false;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int64_t seen = 0;                                                    // graphs added to group `cur` since it became current
  auto flush = [&]() {
    if (cur < 0) return;
    if (tid == 0) s.counts[cur] += seen;
    if (edge) {
      double* p = s.edge_stats + (int64_t)cur * 3 * E2H + cell;
      p[0] = s0;
      p[E2H] = s1;
      p[2 * E2H] = s2;
    } else {
      s.node_stats[(int64_t)cur * NH + cell] = s0;
    }
  };
  // sixteen graphs per round: their values are loaded together (nothing about a load depends on the groups), then added
  // one graph after the other -- the order of the additions is the order of the graphs
  constexpr int U = 16;
  const float* __restrict__ v0 = edge ? w.al : w.en;
  const int64_t pitch = edge ? E2H : NH;
  for (int gb = 0; gb < a.gc; gb += U) {
    float va[U], vm[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t at = (int64_t)min(gb + u, a.gc - 1) * pitch + cell;
      va[u] = v0[at];
      vm[u] = edge ? w.ms[at] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int gl = gb + u;
      if (gl >= a.gc) break;
      const int gm = a.g0 + gl;
      const int g = s.group ? s.group[gm] : 0;
      if ((unsigned)g >= (unsigned)s.num_groups) {                    // skipped, never clamped
        bad = true;
        continue;
      }
      if (skip && !decode_graph(d, gm).use_edges) continue;
      if (g != cur) {                                                  // the running sums of a group live in registers
        flush();
        cur = g;
        seen = 0;
        if (edge) {
          const double* p = s.edge_stats + (int64_t)g * 3 * E2H + cell;
          s0 = p[0];
          s1 = p[E2H];
          s2 = p[2 * E2H];
        } else {
          s0 = s.node_stats[(int64_t)g * NH + cell];
        }
      }
      const double al = va[u];
      ++seen;
      s0 += al;
      if (edge) {
        s1 += al * al;                                                 // exact in fp64: a fused multiply-add changes nothing
        s2 += (double)vm[u];
      }
    }
  }
  flush();
  if (bad && tid == 0) atomicOr(d.err_flag, TECM_BAD_GROUP);
}

bool served(const TecmSpatial& d) {
  if (d.flags == 0) return (d.Cin == 10 || d.Cin == 6) && d.Demb == C - d.Cin;
  return d.flags == TECM_SPATIAL_NO_RESIDUAL && d.Cin == C && d.Demb == 0;
}

// workspace floats of one graph: x_l and x_r rows; alpha, m and the entropy when the statistics are accumulated
int64_t graph_floats(const TecmSpatial& d, const TecmSpatialAttn& a) {
  const int64_t E2 = (int64_t)a.E + d.N;
  return (int64_t)d.N * 2 * CP + (a.edge_stats ? 2 * E2 * H + (int64_t)d.N * H : 0);
}

// graphs per chunk: what fits WS_CHUNK_BYTES, at least one
int64_t chunk_graphs(const TecmSpatial& d, const TecmSpatialAttn& a) {
  const int64_t gc = WS_CHUNK_BYTES / (graph_floats(d, a) * (int64_t)sizeof(float)), G = (int64_t)d.B * d.L;
  return gc < 1 ? 1 : (gc > G ? G : gc);
}

bool fits_32bit(const TecmSpatial& d, const TecmSpatialAttn& a) {       // thread ids are 32-bit (two threads per row)
  return (int64_t)d.N * d.B * d.L < (int64_t)1 << 29 && ((int64_t)a.E + d.N) * H < (int64_t)1 << 30;
}

template <int CIN>
void launch_rows(const AttnArgs& q, hipStream_t st) {
  const int64_t rows = (int64_t)q.gc * q.d.N;
  hipLaunchKernelGGL(spatial_attn_rows_kernel<CIN>, dim3((unsigned)((rows + TB - 1) / TB), 2), dim3(TB), 0, st, q);
}

}  // namespace

// Floats of workspace tecm_spatial_attention asks for by default, or 0 when it does not serve the call.
extern "C" int64_t tecm_spatial_attention_ws_floats(const TecmSpatial* dp, const TecmSpatialAttn* ap) {
  if (dp == nullptr || ap == nullptr || check_common("tecm_spatial_attention_ws_floats", *dp) != TECM_OK || !served(*dp))
    return 0;
  if (ap->E < 0 || !fits_32bit(*dp, *ap)) return 0;
  return chunk_graphs(*dp, *ap) * graph_floats(*dp, *ap);
}

extern "C" int tecm_spatial_attention(const TecmSpatial* dp, const TecmSpatialAttn* ap, void* stream) {
  TECM_REQUIRE(dp != nullptr && ap != nullptr, TECM_E_ARG, "tecm_spatial_attention: null descriptor");
  const TecmSpatial& d = *dp;
  const TecmSpatialAttn& s = *ap;
  const int rc = check_common("tecm_spatial_attention", d);
  if (rc) return rc;
  TECM_REQUIRE(served(d), TECM_E_ARG,
               "tecm_spatial_attention: serves the fused stage (flags = 0, Cin 6 or 10, Demb = 22 - Cin) and the stand-alone "
               "GATv2 (TECM_SPATIAL_NO_RESIDUAL, Cin = 22, Demb = 0) (got flags=%d Cin=%d Demb=%d)",
               d.flags, d.Cin, d.Demb);
  TECM_REQUIRE(s.E >= 0 && fits_32bit(d, s), TECM_E_ARG, "tecm_spatial_attention: bad edge count or too many rows / entries");
  TECM_REQUIRE(s.alpha || s.edge_stats, TECM_E_ARG, "tecm_spatial_attention: neither alpha nor edge_stats: nothing to do");
  TECM_REQUIRE(!s.edge_stats || (s.node_stats && s.counts && s.num_groups > 0), TECM_E_ARG,
               "tecm_spatial_attention: the statistics need edge_stats, node_stats, counts and num_groups > 0");
  TECM_REQUIRE((s.flags & ~TECM_ATTN_SKIP_UNCONNECTED) == 0, TECM_E_ARG, "tecm_spatial_attention: unknown flags %d", s.flags);
  TECM_REQUIRE(s.ws != nullptr, TECM_E_ARG, "tecm_spatial_attention: null workspace");
  const int64_t pg = graph_floats(d, s), G = (int64_t)d.B * d.L;
  const int64_t have = s.ws_floats > 0 ? s.ws_floats : chunk_graphs(d, s) * pg;
  TECM_REQUIRE(have >= pg, TECM_E_ARG, "tecm_spatial_attention: the workspace holds %lld floats, one graph needs %lld",
               (long long)have, (long long)pg);
  TECM_REQUIRE(tecm_aligned(s.ws, 16) && tecm_aligned(d.x, 8), TECM_E_ALIGN,
               "tecm_spatial_attention: the workspace must be 16-byte aligned, x 8-byte aligned");
  TECM_REQUIRE(tecm_aligned(s.alpha, 4) && tecm_aligned(s.perm, 4) && tecm_aligned(s.group, 4) &&
                   tecm_aligned(s.edge_stats, 8) && tecm_aligned(s.node_stats, 8) && tecm_aligned(s.counts, 8),
               TECM_E_ALIGN, "tecm_spatial_attention: alpha, perm and group must be 4-byte, the statistics 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  AttnArgs q;
  q.d = d;
  q.a = s;
  q.gcap = (int)(have / pg > G ? G : have / pg);
  for (int64_t g0 = 0; g0 < G; g0 += q.gcap) {
    q.g0 = (int)g0;
    q.gc = (int)(G - g0 < q.gcap ? G - g0 : q.gcap);
    if (d.Cin == 10) launch_rows<10>(q, st);
    else if (d.Cin == 6) launch_rows<6>(q, st);
    else launch_rows<C>(q, st);
    TECM_CHECK_LAUNCH("tecm_spatial_attention(rows)");
    const int64_t rows = (int64_t)q.gc * d.N;
    hipLaunchKernelGGL(spatial_attn_target_kernel, dim3((unsigned)((2 * rows + TB - 1) / TB)), dim3(TB), 0, st, q);
    TECM_CHECK_LAUNCH("tecm_spatial_attention(target)");
    if (s.edge_stats) {
      const int64_t cells = ((int64_t)s.E + 2 * (int64_t)d.N) * H;
      hipLaunchKernelGGL(spatial_attn_accumulate_kernel, dim3((unsigned)((cells + TB - 1) / TB)), dim3(TB), 0, st, q);
      TECM_CHECK_LAUNCH("tecm_spatial_attention(accumulate)");
    }
  }
  return TECM_OK;
}
