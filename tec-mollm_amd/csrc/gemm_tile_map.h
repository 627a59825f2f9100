// Block -> tile map shared by the bf16 and split-bf16 GEMM kernels (the fp32 gemm_kernel of gemm_impl.h keeps the same
// formula inline: through this function six of its instances spill other numbers of scalar registers): integers only,
// compiled for the device (the kernels) and for the host (util.cpp: tecm_gemm_tile_of_block, which tests/test_host.py
// checks for bijectivity).
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

}  // namespace tecm_gemm
