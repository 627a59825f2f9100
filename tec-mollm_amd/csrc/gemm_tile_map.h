// Block -> tile map shared by the bf16 and split-bf16 GEMM kernels (the fp32 gemm_kernel of gemm_impl.h keeps the same
// formula inline: through this function six of its instances spill other numbers of scalar registers): integers only,
// compiled for the device (the kernels) and for the host (util.cpp: tecm_gemm_tile_of_block, which tests/test_host.py
// checks for bijectivity).  Also the row test of TecmGemm's dead-rectangle / zero-rectangle hints (rows_in_rect: inlined into
// the fp32 kernel, tecm_gemm_rows_in_rect / tecm_gemm_rect_tiles on the host, tests/test_host_causal_q0.py).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TECM_TILE_MAP_FN __host__ __device__ __forceinline__
#else
#define TECM_TILE_MAP_FN inline
#endif

namespace tecm_gemm {

// XCD-aware, bijective: blocks that share an XCD (id % 8) get a contiguous run of the nwg work items, so that what
// neighbours in the run share is re-read from that XCD's L2.
TECM_TILE_MAP_FN int xcd_contiguous(int id, int nwg) {
  const int xcd = id & 7, local = id >> 3;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + local;
}

// (a function, not a bare ?: -- its result is known to be defined, which keeps a `freeze` out of the kernels' address math)
TECM_TILE_MAP_FN int tile_min(int a, int b) { return a < b ? a : b; }

struct TileIdx {
  int tm, tn;
};

// Grouped order inside the XCD's run: group_m m-tiles x all n-tiles per group, m fastest, so the ~64 blocks resident on
// one XCD form a (group_m m) x (n) super-tile whose A and B panels both live in that XCD's 4 MiB L2.  The last group
// holds what is left of tiles_m.  group_m is the caller's: host-tunable through TecmGemm::_p1, with a per-family default.
TECM_TILE_MAP_FN TileIdx tile_of_block(int id, int tiles_m, int tiles_n, int group_m) {
  const int wg = xcd_contiguous(id, tiles_m * tiles_n);
  const int per_group = group_m * tiles_n;
  const int group = wg / per_group;
  const int first_m = group * group_m;
  const int gsz = tile_min(tiles_m - first_m, group_m);
  const int in_group = wg - group * per_group;
  return {first_m + in_group % gsz, in_group / gsz};
}

// The row test of TecmGemm's two hints (include/tecmollm.h): does every row of [r0, r1) have row % period < rows?
// (period > 0, 0 <= r0 < r1 < 2^31.)  The run starts at p = r0 % period and must end before it reaches `rows`; a run that
// wraps around the period passes through [rows, period) unless there is no such gap.  Scalar and per block in the kernels.
TECM_TILE_MAP_FN bool rows_in_rect(long long r0, long long r1, int period, int rows) {
  if (rows >= period) return true;
  const unsigned p = (unsigned)r0 % (unsigned)period;
  return (long long)p + (r1 - r0) <= (long long)rows;
}

// Tiles of bm x bn that lie wholly inside (row % period < rows, col < cols), by their rows inside M and columns inside N.
inline long long rect_tiles(long long M, long long N, int bm, int bn, int period, int rows, long long cols) {
  if (period <= 0 || rows <= 0 || cols <= 0 || M <= 0 || N <= 0 || bm <= 0 || bn <= 0) return 0;
  long long tn = 0, tm = 0;
  for (long long n0 = 0; n0 < N; n0 += bn) tn += (n0 + bn < N ? n0 + bn : N) <= cols;
  for (long long m0 = 0; m0 < M; m0 += bm) tm += rows_in_rect(m0, m0 + bm < M ? m0 + bm : M, period, rows);
  return tm * tn;
}

}  // namespace tecm_gemm
