// Reordering of ensemble members by a dependence template: tecm_member_reorder (include/tecmollm.h (3n)), the kernel under
// tecmollm.coherence.reorder_members -- ensemble copula coupling (the template is a raw ensemble) and the Schaake shuffle (the
// template is K dated rows of an archive, gathered in place).  In every cell (s, h, i) the K values keep their bits and
// move to the member indices in the rank order of the K template values.  A streaming kernel: 2 K floats read and K floats
// written per cell.
//
// Block (x, y, z) = (tile of 64 nodes, horizon h, sample s), ONE wave: lane = node of the tile, so a thread owns one cell and
// every global load and store of the wave runs along the nodes (stride_i == 1 is the coalesced layout, as in ensemble.hip).
//
// The total order of the contract (numbers by <, -0 == +0, NaN behind every number, ties and NaNs by member index) is the
// unsigned order of a 32-bit key made with integer instructions only (order_key), ties by index.  The position of member k
// in that order is counted, not sorted for:  pos_k = k - #{j < k : key_k < key_j} + #{j > k : key_j < key_k},  one compare per
// pair j < k, K (K - 1) / 2 of them, every register index a compile-time constant (the loops over the padded size KP are
// fully unrolled, and a wave-uniform test skips the members k >= K).  The two run-time indices go through a column of LDS
// that only the owning lane touches:
//   values:   pos_k -> lds[pos_k][lane] = v_k            (the cell's values, sorted)
//   template: r_k   -> out[k] = lds[r_k][lane]           (plane k is stored as 64 consecutive floats)
// lds is [KP][64] floats, the bank of an entry is its lane: no conflict, no barrier (one wave, program order), and no
// instance uses scratch (a ceiling of __graft_entry__.py).
//
// out may be the values themselves (same pointer, same strides): a thread has read its K values before it stores one, and
// no other thread touches its cell.
//
// Dated template: the K rows of sample s are wave-uniform, checked before anything is read; a sample with a row outside
// [0, T - H] reads nothing of the series, gets NaN in every output and 255 in every rank, and sets TECM_BAD_ROW.
#include <limits>

#include "common.h"

namespace {

constexpr int MR_TILE = 64;                  // nodes per block = lanes of the wave

// Unsigned order of the keys = the contract's order of the floats: negative numbers ascending, then zero (either sign),
// then positive numbers, +inf, and every NaN at the top.  Integer instructions only: no float mode takes part.
__device__ __forceinline__ uint32_t order_key(uint32_t bits) {
  const uint32_t mag = bits & 0x7fffffffu;
  uint32_t key = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  if (mag == 0u) key = 0x80000000u;
  if (mag > 0x7f800000u) key = 0xffffffffu;
  return key;
}

// pos[k] = position of member k among the K keys, ties by member index
template <int KP>
__device__ __forceinline__ void positions(const uint32_t (&key)[KP], int (&pos)[KP], int K) {
#pragma unroll
  for (int k = 0; k < KP; ++k) pos[k] = k;
#pragma unroll
  for (int k = 1; k < KP; ++k) {
    if (k < K) {
#pragma unroll
      for (int j = 0; j < k; ++j) {
        const int c = key[k] < key[j] ? 1 : 0;   // k goes before j (an equal key stays behind: j < k)
        pos[j] += c;
        pos[k] -= c;
      }
    }
  }
}

template <int KP, bool DATED>
__global__ __launch_bounds__(MR_TILE) void member_reorder_kernel(TecmMemberReorder q) {
  const unsigned lane = threadIdx.x;
  const int64_t h = blockIdx.y, s = blockIdx.z;
  const int64_t i = (int64_t)blockIdx.x * MR_TILE + lane;
  const bool own = i < q.I;
  const int K = q.K;
  __shared__ uint32_t sorted[KP * MR_TILE];  // [position][lane]: a thread touches its own column only

  const int64_t o_cell = s * q.o_stride_s + h * q.o_stride_h + i * q.o_stride_i;
  const int64_t r_cell = (s * q.H + h) * q.I + i;          // out_rank is contiguous (K, S, H, I)
  const int64_t r_plane = q.S * (int64_t)q.H * q.I;

  if constexpr (DATED) {
    bool bad = false;                        // wave-uniform: the rows of sample s
    for (int k = 0; k < K; ++k) {
      const int64_t row = q.rows[s * K + k];
      bad |= row < 0 || row + q.H > q.T;
    }
    if (bad) {
      if (own) {
        const float nan = std::numeric_limits<float>::quiet_NaN();
        for (int k = 0; k < K; ++k) {
          q.out[o_cell + (int64_t)k * q.o_stride_k] = nan;
          if (q.out_rank) q.out_rank[r_cell + (int64_t)k * r_plane] = 255;
        }
      }
      if (blockIdx.x == 0 && blockIdx.y == 0 && lane == 0) atomicOr(q.err_flag, TECM_BAD_ROW);
      return;
    }
  }
  if (!own) return;

  {  // the values, sorted into the lane's column
    const uint32_t* v = reinterpret_cast<const uint32_t*>(q.values) + s * q.v_stride_s + h * q.v_stride_h + i * q.v_stride_i;
    uint32_t bits[KP], key[KP];
    int pos[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      bits[k] = k < K ? v[(int64_t)k * q.v_stride_k] : 0u;
      key[k] = order_key(bits[k]);
    }
    positions<KP>(key, pos, K);
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (k < K) sorted[pos[k] * MR_TILE + lane] = bits[k];
  }

  uint32_t key[KP];
  int pos[KP];
  if constexpr (DATED) {
    const uint32_t* t = reinterpret_cast<const uint32_t*>(q.tmpl) + i * q.t_stride_i;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const int64_t row = k < K ? (int64_t)q.rows[s * K + k] + h : 0;
      key[k] = order_key(k < K ? t[row * q.t_stride_row] : 0u);
    }
  } else {
    const uint32_t* t = reinterpret_cast<const uint32_t*>(q.tmpl) + s * q.t_stride_s + h * q.t_stride_h + i * q.t_stride_i;
#pragma unroll
    for (int k = 0; k < KP; ++k) key[k] = order_key(k < K ? t[(int64_t)k * q.t_stride_k] : 0u);
  }
  positions<KP>(key, pos, K);
  uint32_t* out = reinterpret_cast<uint32_t*>(q.out) + o_cell;
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    if (k < K) {
      out[(int64_t)k * q.o_stride_k] = sorted[pos[k] * MR_TILE + lane];
      if (q.out_rank) q.out_rank[r_cell + (int64_t)k * r_plane] = (uint8_t)pos[k];
    }
  }
}

template <int KP>
void launch(const TecmMemberReorder* r, dim3 grid, hipStream_t stream) {
  if (r->rows) hipLaunchKernelGGL((member_reorder_kernel<KP, true>), grid, dim3(MR_TILE), 0, stream, *r);
  else hipLaunchKernelGGL((member_reorder_kernel<KP, false>), grid, dim3(MR_TILE), 0, stream, *r);
}

// The byte range [lo, hi) an operand of element size `esize` can touch: base + sum n_d * stride_d over 0 <= n_d < dim_d.
struct Span { intptr_t lo, hi; };
Span span_of(const void* base, int esize, const int64_t (&dims)[4], const int64_t (&strides)[4]) {
  int64_t lo = 0, hi = 0;
  for (int d = 0; d < 4; ++d) {
    const int64_t reach = (dims[d] - 1) * strides[d];
    if (reach < 0) lo += reach; else hi += reach;
  }
  const intptr_t b = (intptr_t)base;
  return {b + (intptr_t)lo * esize, b + (intptr_t)(hi + 1) * esize};
}
bool overlap(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }
// |sum n_d * stride_d| of an operand stays below 2^62 elements
bool addressable(const int64_t (&dims)[4], const int64_t (&strides)[4]) {
  long double reach = 0;
  for (int d = 0; d < 4; ++d) reach += (long double)(dims[d] - 1) * fabsl((long double)strides[d]);
  return reach < 4.0e18L;
}

}  // namespace

extern "C" int tecm_member_reorder(const TecmMemberReorder* r, void* stream) {
  TECM_REQUIRE(r, TECM_E_ARG, "tecm_member_reorder: null descriptor");
  TECM_REQUIRE(r->values && r->tmpl && r->out, TECM_E_ARG, "tecm_member_reorder: null pointer");
  TECM_REQUIRE(r->S > 0 && r->H > 0 && r->I > 0, TECM_E_ARG, "tecm_member_reorder: bad shape");
  TECM_REQUIRE(r->K >= 2 && r->K <= TECM_ENS_MAX_K, TECM_E_ARG, "tecm_member_reorder: K = %d outside [2, %d]", (int)r->K,
               TECM_ENS_MAX_K);
  const int64_t tiles = (r->I + MR_TILE - 1) / MR_TILE;
  TECM_REQUIRE(r->S <= TECM_REORDER_MAX_GRID && r->H <= TECM_REORDER_MAX_GRID && tiles <= INT32_MAX, TECM_E_ARG,
               "tecm_member_reorder: S and H must be <= %d and I <= 64 * (2^31 - 1)", TECM_REORDER_MAX_GRID);
  const int64_t dims[4] = {r->K, r->S, r->H, r->I};
  const int64_t vs[4] = {r->v_stride_k, r->v_stride_s, r->v_stride_h, r->v_stride_i};
  const int64_t os[4] = {r->o_stride_k, r->o_stride_s, r->o_stride_h, r->o_stride_i};
  const int64_t rs[4] = {r->S * (int64_t)r->H * r->I, (int64_t)r->H * r->I, r->I, 1};
  TECM_REQUIRE(addressable(dims, vs) && addressable(dims, os) && addressable(dims, rs), TECM_E_ARG,
               "tecm_member_reorder: an operand does not fit 64-bit addressing");
  for (int d = 0; d < 4; ++d)
    TECM_REQUIRE(dims[d] == 1 || os[d] != 0, TECM_E_ARG, "tecm_member_reorder: out has a zero stride: cells would share storage");
  TECM_REQUIRE(tecm_aligned(r->values, 4) && tecm_aligned(r->tmpl, 4) && tecm_aligned(r->out, 4) && tecm_aligned(r->rows, 4),
               TECM_E_ALIGN, "tecm_member_reorder: values, template, rows and out must be 4-byte aligned");
  Span tspan;
  if (r->rows) {
    TECM_REQUIRE(r->err_flag && tecm_aligned(r->err_flag, 4), TECM_E_ARG,
                 "tecm_member_reorder: a dated template needs the 4-byte aligned device error word");
    TECM_REQUIRE(r->T >= r->H, TECM_E_ARG, "tecm_member_reorder: the series has T = %lld rows, fewer than H = %d",
                 (long long)r->T, (int)r->H);
    const int64_t td[4] = {1, 1, r->T, r->I}, ts[4] = {0, 0, r->t_stride_row, r->t_stride_i};
    TECM_REQUIRE(addressable(td, ts), TECM_E_ARG, "tecm_member_reorder: the series does not fit 64-bit addressing");
    tspan = span_of(r->tmpl, 4, td, ts);
    const int64_t rd[4] = {1, 1, r->S, r->K}, rst[4] = {0, 0, r->K, 1};
    TECM_REQUIRE(!overlap(span_of(r->out, 4, dims, os), span_of(r->rows, 4, rd, rst)), TECM_E_ARG,
                 "tecm_member_reorder: out overlaps rows");
  } else {
    const int64_t ts[4] = {r->t_stride_k, r->t_stride_s, r->t_stride_h, r->t_stride_i};
    TECM_REQUIRE(addressable(dims, ts), TECM_E_ARG, "tecm_member_reorder: the template does not fit 64-bit addressing");
    tspan = span_of(r->tmpl, 4, dims, ts);
  }
  // aliasing: out may BE values (same pointer, same strides); every other overlap is refused
  const Span vspan = span_of(r->values, 4, dims, vs), ospan = span_of(r->out, 4, dims, os);
  const bool same = r->out == r->values && vs[0] == os[0] && vs[1] == os[1] && vs[2] == os[2] && vs[3] == os[3];
  TECM_REQUIRE(same || !overlap(ospan, vspan), TECM_E_ARG,
               "tecm_member_reorder: out overlaps values without being the same view (same pointer and strides)");
  TECM_REQUIRE(!overlap(ospan, tspan), TECM_E_ARG, "tecm_member_reorder: out overlaps the template");
  if (r->out_rank) {
    const Span rspan = span_of(r->out_rank, 1, dims, rs);
    TECM_REQUIRE(!overlap(rspan, ospan) && !overlap(rspan, vspan) && !overlap(rspan, tspan), TECM_E_ARG,
                 "tecm_member_reorder: out_rank overlaps another operand");
  }
  const dim3 grid((unsigned)tiles, (unsigned)r->H, (unsigned)r->S);
  hipStream_t st = (hipStream_t)stream;
  if (r->K <= 2) launch<2>(r, grid, st);
  else if (r->K <= 4) launch<4>(r, grid, st);
  else if (r->K <= 8) launch<8>(r, grid, st);
  else if (r->K <= 16) launch<16>(r, grid, st);
  else if (r->K <= 32) launch<32>(r, grid, st);
  else launch<64>(r, grid, st);
  TECM_CHECK_LAUNCH("tecm_member_reorder");
  return TECM_OK;
}
