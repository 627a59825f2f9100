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
extern "C" int tecm_abi_version(void) { return TECM_ABI_VERSION; }

extern "C" void tecm_gemm_tile_of_block(int id, int tiles_m, int tiles_n, int group_m, int* tm, int* tn) {
  const tecm_gemm::TileIdx t = tecm_gemm::tile_of_block(id, tiles_m, tiles_n, group_m);
  *tm = t.tm;
  *tn = t.tn;
}
extern "C" void tecm_gemm_tiles_of_blocks(int tiles_m, int tiles_n, int group_m, int* tm, int* tn) {
  for (int id = 0; id < tiles_m * tiles_n; ++id) tecm_gemm_tile_of_block(id, tiles_m, tiles_n, group_m, tm + id, tn + id);
}
