// Host-side helpers shared by every translation unit of libtecmollm_hip.so.
#include "common.h"
#include "gemm_tile_map.h"
#include <string.h>

static thread_local char g_err[512] = "no error";

void tecm_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* tecm_last_error(void) { return g_err; }

thread_local const char* tecm_gemm_kernel = "";
extern "C" const char* tecm_gemm_last_kernel(void) { return tecm_gemm_kernel; }
thread_local int64_t tecm_gemm_skipped = 0;
extern "C" int64_t tecm_gemm_last_skipped_flops(void) { return tecm_gemm_skipped; }
extern "C" int tecm_abi_version(void) { return TECM_ABI_VERSION; }

extern "C" int tecm_gemm_rows_in_rect(int64_t r0, int64_t r1, int32_t period, int32_t rows) {
  if (period <= 0 || r0 < 0 || r1 <= r0) return 0;
  return tecm_gemm::rows_in_rect(r0, r1, period, rows) ? 1 : 0;
}
extern "C" int64_t tecm_gemm_rect_tiles(int64_t M, int64_t N, int32_t bm, int32_t bn, int32_t period, int32_t rows,
                                        int64_t cols) {
  return tecm_gemm::rect_tiles(M, N, bm, bn, period, rows, cols);
}

extern "C" void tecm_gemm_tile_of_block(int id, int tiles_m, int tiles_n, int group_m, int* tm, int* tn) {
  const tecm_gemm::TileIdx t = tecm_gemm::tile_of_block(id, tiles_m, tiles_n, group_m);
  *tm = t.tm;
  *tn = t.tn;
}
extern "C" void tecm_gemm_tiles_of_blocks(int tiles_m, int tiles_n, int group_m, int* tm, int* tn) {
  for (int id = 0; id < tiles_m * tiles_n; ++id) tecm_gemm_tile_of_block(id, tiles_m, tiles_n, group_m, tm + id, tn + id);
}
