// The causal attention probabilities of one GPT-2 block, handed to the caller (GPT2Attention with output_attentions=True,
// modeling_gpt2.py:144-226, at the reference's call site modules.py:205-209; the forward: attention.hip / attention_long.hip,
// which form them in registers and keep only ctx).  Per (sequence (b, n), head h), from the q and k columns of the layer's qkv,
//     s_ij = (q_i . k_j) / 8        p_ij = exp(s_ij - max_j s_ij) / sum_{j<=i} exp(s_ij - max)        (fp32, j <= i)
// BEFORE the attention dropout (what eval() uses, what training draws its masks over).  The denominator is the sum of exactly
// the numerators that are then divided, so a row sums to 1 within (i + 2) * 2^-24 -- an online (rescaled) denominator would
// not give that bound.  Row 0 is [1, 0, ...] by definition and q_0 is never loaded, at any T (fp32 mode leaves those columns
// unwritten, tecm_attention_reads_q0).  With the probabilities, in float64 from the fp32 p that is (or would be) exported:
// per sequence the mean row entropy, look-back distance, sink weight p_i0 and self weight p_ii, the lag sums
// L_d = sum_i p_{i,i-d}, and for T <= 32 the matrix itself, all summed over sequences per group of windows.
// Two kernels per chunk of windows, no float atomics, every sum in an order fixed by (B, N, T):
//   probs (T <= 32)   16 lanes = one (sequence, head), a float4 of the head dims per lane, the keys register-resident behind
//                     wave-uniform guards (TM = 4, 8, 16, 32).  group16_sum gives every lane every score; lane l keeps the scores
//                     of keys l and l + 16, so max, numerators, denominator and quotient are two registers per lane and
//                     16-lane reductions.  A block is 16 consecutive nodes of one (window, head): their lag sums and matrix rows
//                     meet in LDS and leave as ONE float64 partial per block.
//   probs (T >= 33)   a wave = one (sequence, head), four consecutive nodes per block.  q_i sits in 64 registers, lane l takes
//                     the keys l, l + 64, ..; the row's scores are parked in LDS, become numerators and then probabilities there
//                     (max, sum through wave reductions).  Lane l owns the lags l, l + 64, .. in statically indexed registers
//                     and reads p_{i,i-d} back from the parked row (rows alternate between two LDS buffers: one barrier per
//                     row).  No probability matrix of a window is ever materialised; plain FMAs -- this path explains a forward,
//                     it does not train.
//   accumulate        thread = one cell of node_stats / lag_stats / matrix_stats: walks the windows of the chunk in ascending b,
//                     sums a window's block partials in ascending block order and adds the window to the float64 statistics of
//                     its group with plain loads and stores -- one owner per cell, the same bits whatever the chunking.
// The workspace holds one chunk of whole windows (<= 64 MiB unless one window needs more); the launcher walks the chunks.
#include "common.h"

namespace {

constexpr int SHORT_T = 32;            // largest T of the 16-lane kernels
constexpr int IPB_SHORT = 16;          // (sequence, head) items per block: 16 groups of 16 lanes
constexpr int IPB_LONG = 4;            // ... : 4 waves
constexpr int MAX_T = 1024;
constexpr int64_t WS_CHUNK_BYTES = (int64_t)64 << 20;

struct ProbArgs {
  TecmTemporalAttn d;
  int b0, bc, wcap;                     // windows [b0, b0 + bc); wcap = windows the workspace is laid out for
  int Ns, NB;                           // node slots walked, blocks of IPB slots per (window, head)
  int stats, mat;                       // accumulate; with the matrix
  const int32_t* nodes;                 // slot -> node id, or NULL = identity
  float* probs;                         // NULL: no export in this pass
};

// workspace of a chunk laid out for wcap windows, all doubles: node values (window, 4, N, H) | lag partials (window, block,
// H, T) | matrix partials (window, block, H, T, T)
struct WsLayout {
  double *node, *lag, *mat;
};
__host__ __device__ inline WsLayout ws_layout(const ProbArgs& q) {
  const TecmTemporalAttn& d = q.d;
  WsLayout w;
  w.node = reinterpret_cast<double*>(d.ws);
  w.lag = w.node + (int64_t)q.wcap * 4 * d.N * d.heads;
  w.mat = w.lag + (int64_t)q.wcap * q.NB * d.heads * d.T;
  return w;
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
  return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
}
template <bool Q16>
__device__ __forceinline__ float4 ldq(const float* __restrict__ qkv, int64_t off) {
  if constexpr (Q16) {
    const tecm_bf16x4 h = *reinterpret_cast<const tecm_bf16x4*>(reinterpret_cast<const __bf16*>(qkv) + off);
    return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
  } else {
    return *reinterpret_cast<const float4*>(qkv + off);
  }
}
__device__ __forceinline__ float group16_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double group16_sum_f64(double v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// -p ln p in float64 from the fp32 p (0 ln 0 = 0)
__device__ __forceinline__ double plogp(float p) { return p > 0.f ? -(double)p * log((double)p) : 0.0; }

// (window, node-block, head) of a block and the slot / node of one of its items
struct Item {
  int b, bl, nb, h, slot, n;
  bool in_range, valid;               // slot < Ns; and its node id inside [0, N)
};
__device__ __forceinline__ Item decode_item(const ProbArgs& a, int ipb, int which) {
  Item it;
  int idx = blockIdx.x;
  it.h = idx % a.d.heads;
  idx /= a.d.heads;
  it.nb = idx % a.NB;
  it.bl = idx / a.NB;
  it.b = a.b0 + it.bl;
  it.slot = it.nb * ipb + which;
  it.in_range = it.slot < a.Ns;
  it.n = it.in_range ? (a.nodes ? a.nodes[it.slot] : it.slot) : -1;
  it.valid = it.in_range && (unsigned)it.n < (unsigned)a.d.N;
  return it;
}

// ---- T <= 32: 16 lanes per (sequence, head), keys in registers
template <int TM, bool Q16>
__global__ __launch_bounds__(256) void att_probs_short_kernel(const ProbArgs a) {
  __shared__ float rowS[2][IPB_SHORT][SHORT_T];        // the current row of every item (matrix sums), two rows in flight
  __shared__ double lagS[IPB_SHORT][SHORT_T];
  const TecmTemporalAttn& d = a.d;
  const int T = d.T, N = d.N, H = d.heads, D = d.D;
  const int sub = threadIdx.x & 15, gi = threadIdx.x >> 4, base = threadIdx.x & 48;
  const Item it = decode_item(a, IPB_SHORT, gi);
  const float* __restrict__ qkv = reinterpret_cast<const float*>(d.qkv);
  const int64_t ld = 3 * (int64_t)D;
  const int64_t row0 = (int64_t)it.b * T * N + (it.valid ? it.n : 0);      // an item without a node reads node 0 and adds zeros
  const int col = it.h * 64 + sub * 4;
  float4 k[TM];
#pragma unroll
  for (int p = 0; p < TM; ++p) {
    k[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p < T) k[p] = ldq<Q16>(qkv, (row0 + (int64_t)p * N) * ld + D + col);
  }
  float* out = (a.probs && it.in_range) ? a.probs + (((int64_t)it.b * a.Ns + it.slot) * H + it.h) * T * T : nullptr;
  const WsLayout w = ws_layout(a);
  double* matP = a.mat ? w.mat + (((int64_t)it.bl * a.NB + it.nb) * H + it.h) * T * T : nullptr;
  double ent = 0.0, lb = 0.0, sinkv = 0.0, selfv = 0.0, lag0 = 0.0, lag1 = 0.0;

  // row i of the item: this lane's probabilities of keys sub (p0) and sub + 16 (p1), exact +0 beyond the diagonal
  auto emit = [&](int i, float p0, float p1) {
    if (!it.valid) p0 = p1 = 0.f;
    if (out) {
      if (sub < T) out[(int64_t)i * T + sub] = p0;
      if (sub + 16 < T) out[(int64_t)i * T + sub + 16] = p1;
    }
    if (!a.stats) return;
    ent += plogp(p0) + plogp(p1);
    if (sub <= i) lb += (double)p0 * (double)(i - sub);
    if (sub + 16 <= i) lb += (double)p1 * (double)(i - sub - 16);
    if (sub == 0) sinkv += (double)p0;
    if (sub == (i & 15)) selfv += (double)(i < 16 ? p0 : p1);
    // lags d = sub and sub + 16: p_{i,i-d} is key j = i - sub (or j - 16), held by lane j & 15 of the group
    {
      const int j = i - sub;
      const float a0 = __shfl(p0, base + (j & 15), 64), a1 = __shfl(p1, base + (j & 15), 64);
      if (j >= 0) lag0 += (double)(j < 16 ? a0 : a1);
      if (j >= 16) lag1 += (double)a0;
    }
    if (a.mat) {
      float(*rs)[SHORT_T] = rowS[i & 1];
      rs[gi][sub] = p0;
      rs[gi][sub + 16] = p1;
      __syncthreads();
      if (threadIdx.x < T) {
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < IPB_SHORT; ++g) s += (double)rs[g][threadIdx.x];
        matP[(int64_t)i * T + threadIdx.x] = s;
      }
    }
  };

  emit(0, sub == 0 ? 1.f : 0.f, 0.f);                       // row 0: one key, p = 1; q_0 is not loaded
  for (int i = 1; i < T; ++i) {
    const float4 qi = ldq<Q16>(qkv, (row0 + (int64_t)i * N) * ld + col);
    float s0 = -INFINITY, s1 = -INFINITY;
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      if (j <= i) {                                          // wave-uniform
        const float s = group16_sum(dot4(qi, k[j])) * 0.125f;
        if ((j & 15) == sub) {
          if (j < 16) s0 = s;
          else s1 = s;
        }
      }
    }
    const bool v0 = sub <= i, v1 = sub + 16 <= i;
    const float mx = group16_max(fmaxf(s0, s1));
    const float e0 = v0 ? expf(s0 - mx) : 0.f, e1 = v1 ? expf(s1 - mx) : 0.f;
    const float den = group16_sum(e0 + e1);                  // a key beyond the diagonal adds an exact zero
    emit(i, v0 ? e0 / den : 0.f, v1 ? e1 / den : 0.f);
  }
  if (!a.stats) return;
  ent = group16_sum_f64(ent);
  lb = group16_sum_f64(lb);
  sinkv = group16_sum_f64(sinkv);
  selfv = group16_sum_f64(selfv);
  if (sub == 0 && it.valid) {
    const int64_t NH = (int64_t)N * H;
    double* p = w.node + (int64_t)it.bl * 4 * NH + (int64_t)it.n * H + it.h;
    const double inv = (double)T;
    p[0] = ent / inv;
    p[NH] = lb / inv;
    p[2 * NH] = sinkv / inv;
    p[3 * NH] = selfv / inv;
  }
  lagS[gi][sub] = lag0;
  lagS[gi][sub + 16] = lag1;
  __syncthreads();
  if (threadIdx.x < T) {
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < IPB_SHORT; ++g) s += lagS[g][threadIdx.x];
    w.lag[(((int64_t)it.bl * a.NB + it.nb) * H + it.h) * T + threadIdx.x] = s;
  }
}

// ---- 33 <= T <= 1024: a wave per (sequence, head)
template <bool Q16>
__global__ __launch_bounds__(256) void att_probs_long_kernel(const ProbArgs a) {
  // per wave two rows of <= 1024 floats; after the last row the same bytes hold the waves' lag sums as doubles
  __shared__ __attribute__((aligned(16))) float scS[IPB_LONG * 2 * MAX_T];
  const TecmTemporalAttn& d = a.d;
  const int T = d.T, N = d.N, H = d.heads, D = d.D;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const Item it = decode_item(a, IPB_LONG, wv);
  const float* __restrict__ qkv = reinterpret_cast<const float*>(d.qkv);
  const int64_t ld = 3 * (int64_t)D;
  const int64_t row0 = (int64_t)it.b * T * N + (it.valid ? it.n : 0);
  const int col = it.h * 64;
  float* out = (a.probs && it.in_range) ? a.probs + (((int64_t)it.b * a.Ns + it.slot) * H + it.h) * T * T : nullptr;
  double ent = 0.0, lb = 0.0, sinkv = 0.0, selfv = 0.0;
  double lag[MAX_T / 64];                                   // lags lane + 64 m, statically indexed
#pragma unroll
  for (int m = 0; m < MAX_T / 64; ++m) lag[m] = 0.0;
  // row 0: p = [1, 0, ...]; q_0 is not loaded
  if (out)
    for (int j = lane; j < T; j += 64) out[j] = (j == 0 && it.valid) ? 1.f : 0.f;
  if (lane == 0 && it.valid) sinkv = selfv = lag[0] = 1.0;
  for (int i = 1; i < T; ++i) {
    float* sc = scS + (wv * 2 + (i & 1)) * MAX_T;
    float4 q[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) q[c] = ldq<Q16>(qkv, (row0 + (int64_t)i * N) * ld + col + 4 * c);
    float mx = -INFINITY;
    for (int j = lane; j <= i; j += 64) {
      const int64_t kr = (row0 + (int64_t)j * N) * ld + D + col;
      float4 kk[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) kk[c] = ldq<Q16>(qkv, kr + 4 * c);
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < 16; ++c) s += dot4(q[c], kk[c]);
      s *= 0.125f;
      sc[j] = s;
      mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j <= i; j += 64) {
      const float e = expf(sc[j] - mx);
      sc[j] = e;
      sum += e;
    }
    const float den = wave_sum(sum);
    for (int j = lane; j < T; j += 64) {
      float p = 0.f;
      if (j <= i) {
        p = it.valid ? sc[j] / den : 0.f;
        sc[j] = p;
        if (a.stats) {
          ent += plogp(p);
          lb += (double)p * (double)(i - j);
          if (j == 0) sinkv += (double)p;
          if (j == i) selfv += (double)p;
        }
      }
      if (out) out[(int64_t)i * T + j] = p;
    }
    __syncthreads();                                         // the row is parked: every lane of the wave sees it
    if (a.stats) {
#pragma unroll
      for (int m = 0; m < MAX_T / 64; ++m) {
        if (64 * m <= i) {                                   // wave-uniform
          const int dd = lane + 64 * m;
          if (dd <= i) lag[m] += (double)sc[i - dd];
        }
      }
    }
  }
  if (!a.stats) return;
  ent = wave_sum_f64(ent);
  lb = wave_sum_f64(lb);
  sinkv = wave_sum_f64(sinkv);
  selfv = wave_sum_f64(selfv);
  const WsLayout w = ws_layout(a);
  if (lane == 0 && it.valid) {
    const int64_t NH = (int64_t)N * H;
    double* p = w.node + (int64_t)it.bl * 4 * NH + (int64_t)it.n * H + it.h;
    const double inv = (double)T;
    p[0] = ent / inv;
    p[NH] = lb / inv;
    p[2 * NH] = sinkv / inv;
    p[3 * NH] = selfv / inv;
  }
  __syncthreads();                                           // the last row's lag reads are done: reuse the buffer
  double* lagD = reinterpret_cast<double*>(scS);             // (wave, MAX_T)
#pragma unroll
  for (int m = 0; m < MAX_T / 64; ++m)
    if (lane + 64 * m < T) lagD[wv * MAX_T + lane + 64 * m] = lag[m];
  __syncthreads();
  for (int t = threadIdx.x; t < T; t += 256) {
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < IPB_LONG; ++g) s += lagD[g * MAX_T + t];
    w.lag[(((int64_t)it.bl * a.NB + it.nb) * H + it.h) * T + t] = s;
  }
}

// ---- accumulate: thread = one cell of (4, N, H) | (H, T) | (H, T, T); thread 0 also counts
__global__ __launch_bounds__(256) void att_probs_accumulate_kernel(const ProbArgs a) {
  const TecmTemporalAttn& d = a.d;
  const int64_t NH4 = (int64_t)4 * d.N * d.heads, HT = (int64_t)d.heads * d.T, HTT = a.mat ? HT * d.T : 0;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (tid >= NH4 + HT + HTT) return;
  const int kind = tid < NH4 ? 0 : (tid < NH4 + HT ? 1 : 2);
  const int64_t cell = kind == 0 ? tid : (kind == 1 ? tid - NH4 : tid - NH4 - HT);
  const int64_t cells = kind == 0 ? NH4 : (kind == 1 ? HT : HTT);
  double* dst = kind == 0 ? d.node_stats : (kind == 1 ? d.lag_stats : d.matrix_stats);
  const WsLayout w = ws_layout(a);
  const double* src = kind == 0 ? w.node : (kind == 1 ? w.lag : w.mat);
  const bool count = tid == 0 && (d.flags & TECM_TATT_COUNT);
  int cur = -1;
  bool bad = false;
  double s = 0.0;
  int64_t seen = 0;
  auto at = [&](int g) { return dst + ((int64_t)g * d.num_layers + d.layer) * cells + cell; };
  auto flush = [&]() {
    if (cur < 0) return;
    *at(cur) = s;
    if (count) d.counts[cur] += seen;
  };
  for (int bl = 0; bl < a.bc; ++bl) {
    const int g = d.group ? d.group[a.b0 + bl] : 0;
    if ((unsigned)g >= (unsigned)d.num_groups) {             // skipped, never clamped
      bad = true;
      continue;
    }
    double v;
    if (kind == 0) {
      v = src[(int64_t)bl * NH4 + cell];
    } else {                                                 // the window's block partials, in ascending block order
      const double* p = src + (int64_t)bl * a.NB * cells + cell;
      v = 0.0;
      constexpr int U = 16;                                  // sixteen loads in flight, the additions still one after the other
      for (int nb = 0; nb < a.NB; nb += U) {
        double t[U];
#pragma unroll
        for (int u = 0; u < U; ++u) t[u] = nb + u < a.NB ? p[(int64_t)(nb + u) * cells] : 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (nb + u < a.NB) v += t[u];
      }
    }
    if (g != cur) {                                          // the running sum of a group lives in a register
      flush();
      cur = g;
      seen = 0;
      s = *at(g);
    }
    s += v;
    ++seen;
  }
  flush();
  if (bad && tid == 0) atomicOr(d.err_flag, TECM_BAD_GROUP);
}

int ipb_of(int T) { return T <= SHORT_T ? IPB_SHORT : IPB_LONG; }

const char* refuse(const TecmTemporalAttn& d) {               // NULL: served
  if (d.B < 1 || d.N < 1 || d.heads < 1 || d.D < 1) return "B, N, heads and D must be positive";
  if (d.T < 1 || d.T > MAX_T) return "1 <= T <= 1024 (GPT-2's positions)";
  if (d.D % d.heads != 0 || d.D / d.heads != 64) return "head_dim = D / heads must be 64";
  if (!d.probs && !d.node_stats) return "neither probs nor node_stats: nothing to do";
  if (d.matrix_stats && d.T > SHORT_T) return "matrix_stats is served for T <= 32 only";
  if (d.matrix_stats && !d.node_stats) return "matrix_stats needs the other statistics";
  if (d.nodes && d.Ns < 1) return "nodes needs Ns >= 1";
  const int64_t slots = d.nodes && !d.node_stats ? d.Ns : d.N;
  const int64_t blocks = (int64_t)d.B * ((slots + IPB_LONG - 1) / IPB_LONG) * d.heads;
  if (blocks >= (int64_t)1 << 31 || (int64_t)d.B * d.T * d.N >= (int64_t)1 << 31) return "too many rows or blocks";
  return nullptr;
}

// workspace doubles of one window
int64_t window_doubles(const TecmTemporalAttn& d) {
  const int64_t NB = ((int64_t)d.N + ipb_of(d.T) - 1) / ipb_of(d.T);
  return (int64_t)4 * d.N * d.heads + NB * d.heads * d.T * (d.matrix_stats ? (int64_t)d.T + 1 : 1);
}

int64_t chunk_windows(const TecmTemporalAttn& d) {
  const int64_t wc = WS_CHUNK_BYTES / (window_doubles(d) * (int64_t)sizeof(double));
  return wc < 1 ? 1 : (wc > d.B ? d.B : wc);
}

template <bool Q16>
void launch_probs(const ProbArgs& q, hipStream_t st) {
  const int T = q.d.T;
  const dim3 grid((unsigned)((int64_t)q.bc * q.NB * q.d.heads)), block(256);
  if (T <= 4) hipLaunchKernelGGL((att_probs_short_kernel<4, Q16>), grid, block, 0, st, q);
  else if (T <= 8) hipLaunchKernelGGL((att_probs_short_kernel<8, Q16>), grid, block, 0, st, q);
  else if (T <= 16) hipLaunchKernelGGL((att_probs_short_kernel<16, Q16>), grid, block, 0, st, q);
  else if (T <= SHORT_T) hipLaunchKernelGGL((att_probs_short_kernel<32, Q16>), grid, block, 0, st, q);
  else hipLaunchKernelGGL((att_probs_long_kernel<Q16>), grid, block, 0, st, q);
}

}  // namespace

extern "C" int64_t tecm_temporal_attention_ws_floats(const TecmTemporalAttn* ap) {
  if (ap == nullptr || refuse(*ap) != nullptr) return 0;
  if (!ap->node_stats) return 4;
  return chunk_windows(*ap) * window_doubles(*ap) * 2;
}

extern "C" int tecm_temporal_attention(const TecmTemporalAttn* ap, void* stream) {
  TECM_REQUIRE(ap != nullptr, TECM_E_ARG, "tecm_temporal_attention: null descriptor");
  const TecmTemporalAttn& d = *ap;
  const char* why = refuse(d);
  TECM_REQUIRE(why == nullptr, TECM_E_ARG, "tecm_temporal_attention: %s (got B=%d T=%d N=%d heads=%d D=%d)", why, d.B, d.T, d.N,
               d.heads, d.D);
  TECM_REQUIRE(d.qkv != nullptr, TECM_E_ARG, "tecm_temporal_attention: null qkv");
  TECM_REQUIRE((d.flags & ~(TECM_ATT_QKV_BF16 | TECM_TATT_COUNT)) == 0, TECM_E_ARG, "tecm_temporal_attention: unknown flags %d",
               d.flags);
  const bool q16 = (d.flags & TECM_ATT_QKV_BF16) != 0, stats = d.node_stats != nullptr;
  TECM_REQUIRE(tecm_aligned(d.qkv, q16 ? 8 : 16) && tecm_aligned(d.probs, 4) && tecm_aligned(d.nodes, 4) &&
                   tecm_aligned(d.group, 4),
               TECM_E_ALIGN, "tecm_temporal_attention: qkv must be 16-byte (bf16: 8-byte), probs, nodes and group 4-byte aligned");
  int64_t wcap = d.B;
  if (stats) {
    TECM_REQUIRE(d.lag_stats && d.counts && d.err_flag && d.num_groups > 0 && d.num_layers > 0 && d.layer >= 0 &&
                     d.layer < d.num_layers,
                 TECM_E_ARG, "tecm_temporal_attention: the statistics need node_stats, lag_stats, counts, err_flag, "
                 "num_groups > 0 and 0 <= layer < num_layers");
    TECM_REQUIRE(d.ws != nullptr, TECM_E_ARG, "tecm_temporal_attention: null workspace");
    TECM_REQUIRE(tecm_aligned(d.ws, 16) && tecm_aligned(d.node_stats, 8) && tecm_aligned(d.lag_stats, 8) &&
                     tecm_aligned(d.matrix_stats, 8) && tecm_aligned(d.counts, 8) && tecm_aligned(d.err_flag, 4),
                 TECM_E_ALIGN, "tecm_temporal_attention: the workspace must be 16-byte, the statistics 8-byte aligned");
    const int64_t pw = window_doubles(d) * 2;
    const int64_t have = d.ws_floats > 0 ? d.ws_floats : chunk_windows(d) * pw;
    TECM_REQUIRE(have >= pw, TECM_E_ARG, "tecm_temporal_attention: the workspace holds %lld floats, one window needs %lld",
                 (long long)have, (long long)pw);
    wcap = have / pw > d.B ? d.B : have / pw;
  }
  hipStream_t st = (hipStream_t)stream;
  ProbArgs q;
  q.d = d;
  q.stats = stats ? 1 : 0;
  q.mat = d.matrix_stats ? 1 : 0;
  const int ipb = ipb_of(d.T);
  // the statistics walk every node; an export of a node list alone walks the list, next to the statistics it is a pass of
  // its own
  const bool split = stats && d.probs && d.nodes;
  if (stats) {
    q.wcap = (int)wcap;
    q.Ns = d.N;
    q.NB = (d.N + ipb - 1) / ipb;
    q.nodes = nullptr;
    q.probs = split ? nullptr : d.probs;
    const int64_t cells = (int64_t)4 * d.N * d.heads + (int64_t)d.heads * d.T * (q.mat ? (int64_t)d.T + 1 : 1);
    for (int64_t b0 = 0; b0 < d.B; b0 += wcap) {
      q.b0 = (int)b0;
      q.bc = (int)(d.B - b0 < wcap ? d.B - b0 : wcap);
      if (q16) launch_probs<true>(q, st);
      else launch_probs<false>(q, st);
      TECM_CHECK_LAUNCH("tecm_temporal_attention(probs)");
      hipLaunchKernelGGL(att_probs_accumulate_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, q);
      TECM_CHECK_LAUNCH("tecm_temporal_attention(accumulate)");
    }
  }
  if (!stats || split) {
    q.stats = q.mat = 0;
    q.wcap = d.B;
    q.Ns = d.nodes ? d.Ns : d.N;
    q.NB = (q.Ns + ipb - 1) / ipb;
    q.nodes = d.nodes;
    q.probs = d.probs;
    q.b0 = 0;
    q.bc = d.B;
    if (q16) launch_probs<true>(q, st);
    else launch_probs<false>(q, st);
    TECM_CHECK_LAUNCH("tecm_temporal_attention(export)");
  }
  return TECM_OK;
}
