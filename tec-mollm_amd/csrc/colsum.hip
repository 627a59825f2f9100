// Column sums of the TEC-MoLLM path (gfx950, wave = 64): bias / gamma / beta / wpe gradients and the per-block partial rows
// the LayerNorm and GroupNorm backwards leave behind (layernorm.hip, groupnorm.hip).  Two stages, every sum in a fixed order:
// no atomics, deterministic.
#include "norm_common.h"

namespace {

// ------------------------------------------------------------------------------ column sums
// stage 1: grid (colblocks, RB, nseg).  Lane = column, the 4 waves stride the block's row chunk.
// (the body is shared with colsum_stage1_batch below: rb / s / RB are the block's row chunk, segment and chunk count)
__device__ __forceinline__ void colsum_stage1_body(const float* __restrict__ in, int64_t ld, int64_t outer, int64_t inner,
                                                   int nseg, int C, DropCtxN idc, float* __restrict__ ws, int64_t chunk,
                                                   int rb, int s, int RB) {
  seed_now(idc);
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int64_t total = outer * inner;
  const int64_t beg = (int64_t)rb * chunk;
  const int64_t end = beg + chunk < total ? beg + chunk : total;
  float acc = 0.f;
  if (c < C) {
    float a4[4] = {0.f, 0.f, 0.f, 0.f};          // four rows in flight per wave: the loop is latency-bound otherwise
    for (int64_t r0 = beg + wave; r0 < end; r0 += 16) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t ri = r0 + 4 * u;
        if (ri < end) {
          const int64_t o = ri / inner, j = ri - o * inner;
          const int64_t row = (o * nseg + s) * inner + j;
          float v = in[row * ld + c];
          if (idc.thresh) v *= tecm_drop_mult(idc.seed, (uint64_t)(row * idc.ld + c), idc.thresh, idc.inv);
          a4[u] += v;
        }
      }
    }
    acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && c < C)
    ws[((int64_t)s * RB + rb) * C + c] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}
__global__ __launch_bounds__(256) void colsum_stage1(const float* __restrict__ in, int64_t ld, int64_t outer,
                                                     int64_t inner, int nseg, int C, DropCtxN idc,
                                                     float* __restrict__ ws, int64_t chunk) {
  colsum_stage1_body(in, ld, outer, inner, nseg, C, idc, ws, chunk, blockIdx.y, blockIdx.z, gridDim.y);
}
// Several matrices of the same (rows, C) shape in ONE launch: blockIdx.z picks the matrix from a pointer table in the
// kernel arguments; per matrix the blocks, the row chunks and the order of every sum are those of colsum_stage1 /
// colsum_stage2 on that matrix alone (the LayerNorm backwards' gamma / beta partials: 2 * layers + 1 buffers a step).
constexpr int COLSUM_BATCH_MAX = 32;
struct ColsumBatch {
  const float* in[COLSUM_BATCH_MAX];
  float* out[COLSUM_BATCH_MAX];
};
__global__ __launch_bounds__(256) void colsum_stage1_batch(ColsumBatch tab, int64_t ld, int64_t rows, int C,
                                                           float* __restrict__ ws, int64_t chunk) {
  const int z = blockIdx.z, RB = gridDim.y;
  colsum_stage1_body(tab.in[z], ld, rows, 1, 1, C, DropCtxN{}, ws + (int64_t)z * RB * C, chunk, blockIdx.y, 0, RB);
}

// stage 1, float4 form for 16-byte friendly inputs: a block owns a chunk of rows and ALL C columns,
// thread = (row slot, column quad), so a wave reads whole 1 KiB runs of consecutive rows instead of 256-byte
// slivers (narrow matrices -- 24 .. 128 columns -- ran at 0.3 .. 1 TB/s through the lane-per-column kernel).
__global__ __launch_bounds__(256) void colsum_stage1_v4(const float* __restrict__ in, int64_t ld, int64_t outer,
                                                        int64_t inner, int nseg, int C, DropCtxN idc,
                                                        float* __restrict__ ws, int64_t chunk,
                                                        __bf16* __restrict__ twin = nullptr, int64_t ld_twin = 0) {
  seed_now(idc);
  __shared__ float4 red[256];
  const int Q = C >> 2;                       // quads per row (host: Q <= 256)
  const int RPB = 256 / Q;                    // row slots per pass
  const int q = threadIdx.x % Q, rs = threadIdx.x / Q;
  const int rb = blockIdx.x, s = blockIdx.y;
  const int64_t total = outer * inner;
  const int64_t beg = (int64_t)rb * chunk;
  const int64_t end = beg + chunk < total ? beg + chunk : total;
  float4 a[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (rs < RPB) {
    for (int64_t r0 = beg + rs; r0 < end; r0 += 4 * RPB) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t ri = r0 + (int64_t)u * RPB;
        if (ri < end) {
          int64_t row = ri;
          if (nseg > 1) {
            const int64_t o = ri / inner, j = ri - o * inner;
            row = (o * nseg + s) * inner + j;
          }
          float4 v = *reinterpret_cast<const float4*>(in + row * ld + 4 * q);
          if (idc.thresh) {
            const uint64_t di = (uint64_t)(row * idc.ld + 4 * q);
            v.x *= tecm_drop_mult(idc.seed, di, idc.thresh, idc.inv);
            v.y *= tecm_drop_mult(idc.seed, di + 1, idc.thresh, idc.inv);
            v.z *= tecm_drop_mult(idc.seed, di + 2, idc.thresh, idc.inv);
            v.w *= tecm_drop_mult(idc.seed, di + 3, idc.thresh, idc.inv);
          }
          // every row is visited exactly once: the (masked) values can leave as a bf16 twin on the way (tecm_colsum_twin)
          if (twin) tecm_store_bf16x4(twin + row * ld_twin + 4 * q, v.x, v.y, v.z, v.w);
          a[u].x += v.x; a[u].y += v.y; a[u].z += v.z; a[u].w += v.w;
        }
      }
    }
  }
  float4 t;
  t.x = (a[0].x + a[1].x) + (a[2].x + a[3].x);
  t.y = (a[0].y + a[1].y) + (a[2].y + a[3].y);
  t.z = (a[0].z + a[1].z) + (a[2].z + a[3].z);
  t.w = (a[0].w + a[1].w) + (a[2].w + a[3].w);
  red[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x < Q) {
    float4 acc = red[threadIdx.x];
    for (int r = 1; r < RPB; ++r) {
      const float4 v = red[r * Q + threadIdx.x];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    *reinterpret_cast<float4*>(ws + ((int64_t)s * gridDim.x + rb) * C + 4 * threadIdx.x) = acc;
  }
}

// stage 2: 512 threads = 8 waves per 64 columns, 32 loads in flight per lane: 1024 partial rows are four rounds of
// memory latency (the first version -- 4 waves, 16 in flight -- took sixteen: 23 us per launch, 68 launches a step).
// WAVES = 16 (round 5): the narrow matrices (C <= 128: one or two column blocks for up to 1024 partial rows) take ONE round
// of latency instead of four -- 17-23 us -> see DESIGN_HISTORY B.11; the summation order differs between the two forms
// only in the association of the partial rows, fixed per (RB, WAVES): results stay run-to-run identical.
template <int WAVES>
__device__ __forceinline__ void colsum_stage2_body(const float* __restrict__ ws, int RB, int C, float* __restrict__ out,
                                                   int64_t ldo, int accumulate, float scale, int s) {
  constexpr int UNR = WAVES == 16 ? 64 : 32;            // loads in flight per lane
  __shared__ float red[WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  float acc = 0.f;
  if (c < C) {
    float a32[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) a32[u] = 0.f;
    for (int rb = wave; rb < RB; rb += WAVES * UNR) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) {                   // clamped row + select, not `if`: the bound is wave-uniform, a branch
        const int r = rb + WAVES * u;                   // per load would put a wait between every two of them
        const float v = ws[((int64_t)s * RB + (r < RB ? r : RB - 1)) * C + c];
        a32[u] += r < RB ? v : 0.f;
      }
    }
#pragma unroll
    for (int u = UNR / 2; u > 0; u >>= 1)
#pragma unroll
      for (int v = 0; v < u; ++v) a32[v] += a32[v + u];
    acc = a32[0];
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && c < C) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; w += 4) v += (red[w][lane] + red[w + 1][lane]) + (red[w + 2][lane] + red[w + 3][lane]);
    v *= scale;
    float* o = out + (int64_t)s * ldo + c;
    *o = accumulate ? *o + v : v;
  }
}
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void colsum_stage2(const float* __restrict__ ws, int RB, int nseg, int C,
                                                            float* __restrict__ out, int64_t ldo, int accumulate,
                                                            float scale) {
  colsum_stage2_body<WAVES>(ws, RB, C, out, ldo, accumulate, scale, blockIdx.y);
}
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void colsum_stage2_batch(ColsumBatch tab, const float* __restrict__ ws, int RB, int C) {
  const int z = blockIdx.y;
  colsum_stage2_body<WAVES>(ws + (int64_t)z * RB * C, RB, C, tab.out[z], C, 0, 1.0f, 0);
}
void launch_colsum_stage2(const float* ws, int RB, int nseg, int C, float* out, int64_t ldo, int accumulate, float scale,
                          int colblocks, int waves, hipStream_t st) {
  if (waves == 16)
    hipLaunchKernelGGL(colsum_stage2<16>, dim3(colblocks, nseg), dim3(1024), 0, st, ws, RB, nseg, C, out, ldo, accumulate, scale);
  else
    hipLaunchKernelGGL(colsum_stage2<8>, dim3(colblocks, nseg), dim3(512), 0, st, ws, RB, nseg, C, out, ldo, accumulate, scale);
}

// ------------------------------------------------------------------------------ routing: which kernels serve a call
// Decided here and nowhere else: tecm_colsum / tecm_colsum_twin, tecm_colsum_batch and tecm_colsum_path all ask colsum_plan.
// CS_SCALAR: colsum_stage1 (lane = column); CS_V4: colsum_stage1_v4 (thread = row slot x column quad); CS_BATCH:
// colsum_stage1_batch (CS_SCALAR's blocks and chunks per matrix, a grid dimension walks the pointer table)
enum ColsumStage1 { CS_NONE, CS_SCALAR, CS_V4, CS_BATCH };
struct ColsumPlan {
  ColsumStage1 stage1 = CS_NONE;                 // CS_NONE: refused
  int colblocks = 0;                             // 64-column blocks of the second stage (and of CS_SCALAR / CS_BATCH)
  int64_t rb = 0, chunk = 0;                     // partial rows per segment, rows of the input per partial row
  int waves = 0;                                 // WAVES of colsum_stage2 / colsum_stage2_batch
};
// does the float4 first stage serve the matrix?  (in16: the input AND the workspace are 16-byte aligned)
bool colsum_v4_ok(int64_t ld, int C, bool in16) { return C % 4 == 0 && C <= 1024 && ld % 4 == 0 && in16; }
// total = outer * inner rows per segment; batch: the plan of tecm_colsum_batch's own pair of launches (nseg = 1)
ColsumPlan colsum_plan(int64_t ld, int64_t total, int nseg, int C, bool in16, bool batch) {
  ColsumPlan p;
  if (!(total > 0 && nseg > 0 && C > 0)) return p;
  p.colblocks = (C + 63) / 64;
  if (!batch && colsum_v4_ok(ld, C, in16)) {
    int64_t rb4 = 1024 / nseg;                          // workspace contract: >= 1024 * nseg * C floats
    // at least 16 rows per block.  (Fewer, larger blocks to shrink the second stage were measured at B = 2 -- where the two
    // stages of the 17 column sums are 0.35 ms of a 5.2 ms step: 512 rows per block 5.20 -> 5.85 ms, 2048 -> 7.9 ms, 16 instead
    // of 64 -0.03 ms: the first stage lives on its block count.)  TECM_COLSUM_MINROWS overrides (diagnostics).
    static const int64_t min_rows = [] { const char* e = std::getenv("TECM_COLSUM_MINROWS"); return e ? std::atoll(e) : 16ll; }();
    if (rb4 > (total + min_rows - 1) / min_rows) rb4 = (total + min_rows - 1) / min_rows;
    if (rb4 < 1) rb4 = 1;
    p.chunk = (total + rb4 - 1) / rb4;
    p.rb = (total + p.chunk - 1) / p.chunk;
    p.stage1 = CS_V4;
  } else {
    int64_t rb = 1024 / ((int64_t)p.colblocks * nseg);
    if (rb > 256) rb = 256;
    if (rb > (total + 15) / 16) rb = (total + 15) / 16;
    if (rb < 1) rb = 1;
    p.chunk = (total + rb - 1) / rb;
    p.rb = (total + p.chunk - 1) / p.chunk;
    p.stage1 = batch ? CS_BATCH : CS_SCALAR;
  }
  p.waves = p.colblocks * nseg <= 4 && p.rb > 256 ? 16 : 8;
  return p;
}

}  // namespace

static int colsum_impl(const float* in, int64_t ld, int64_t outer, int64_t inner, int32_t nseg, int32_t C, float* out,
                       int64_t ldo, int32_t accumulate, float scale, const TecmDrop* in_drop, float* workspace, void* twin,
                       int64_t ld_twin, void* stream) {
  TECM_REQUIRE(in && out && workspace, TECM_E_ARG, "tecm_colsum: null pointer");
  TECM_REQUIRE(outer > 0 && inner > 0 && nseg > 0 && C > 0, TECM_E_ARG, "tecm_colsum: bad shape");
  const ColsumPlan p = colsum_plan(ld, outer * inner, nseg, C, tecm_aligned(in, 16) && tecm_aligned(workspace, 16), false);
  hipStream_t st = (hipStream_t)stream;
  const DropCtxN idc = make_dropn(in_drop);
  if (p.stage1 == CS_V4) {
    hipLaunchKernelGGL(colsum_stage1_v4, dim3((unsigned)p.rb, nseg), dim3(256), 0, st, in, ld, outer, inner, nseg, C,
                       idc, workspace, p.chunk, static_cast<__bf16*>(twin), ld_twin);
    TECM_CHECK_LAUNCH("tecm_colsum/stage1_v4");
    launch_colsum_stage2(workspace, (int)p.rb, nseg, C, out, ldo, accumulate, scale, p.colblocks, p.waves, st);
    TECM_CHECK_LAUNCH("tecm_colsum/stage2");
    return TECM_OK;
  }
  TECM_REQUIRE(!twin, TECM_E_ALIGN, "tecm_colsum_twin: needs C %% 4 == 0, C <= 1024 and 16-byte friendly rows");
  hipLaunchKernelGGL(colsum_stage1, dim3(p.colblocks, (unsigned)p.rb, nseg), dim3(256), 0, st, in, ld, outer, inner, nseg,
                     C, idc, workspace, p.chunk);
  TECM_CHECK_LAUNCH("tecm_colsum/stage1");
  launch_colsum_stage2(workspace, (int)p.rb, nseg, C, out, ldo, accumulate, scale, p.colblocks, p.waves, st);
  TECM_CHECK_LAUNCH("tecm_colsum/stage2");
  return TECM_OK;
}

// The route of a call without launching it: "v4 rb=1024 chunk=17 waves=16" -- first stage (scalar: colsum_stage1, v4:
// colsum_stage1_v4, batch: colsum_stage1_batch), partial rows per segment, input rows per partial row, WAVES of the second
// stage; "" where the launcher refuses.  nbuf == 0: tecm_colsum; nbuf > 0: tecm_colsum_batch of nbuf matrices (outer rows,
// inner = nseg = 1), "batch ... launches=2" for its own pair(s) of launches, "each v4 ..." where every matrix goes through
// tecm_colsum one by one.  in_misalign_bytes: distance of the input from a 16-byte boundary (batch: of its best aligned
// matrix, which decides for all); the workspace is taken to be aligned.  Pure host function; the string lives until this
// thread's next call.
extern "C" const char* tecm_colsum_path(int64_t ld, int64_t outer, int64_t inner, int32_t nseg, int32_t C,
                                        int32_t in_misalign_bytes, int32_t nbuf) {
  static thread_local char buf[96];
  static const char* const names[] = {"", "scalar", "v4", "batch"};
  buf[0] = 0;
  if (!(outer > 0 && inner > 0 && nseg > 0 && C > 0 && nbuf >= 0)) return buf;
  const bool in16 = in_misalign_bytes % 16 == 0;
  if (nbuf == 0) {
    const ColsumPlan p = colsum_plan(ld, outer * inner, nseg, C, in16, false);
    std::snprintf(buf, sizeof buf, "%s rb=%lld chunk=%lld waves=%d", names[p.stage1], (long long)p.rb, (long long)p.chunk, p.waves);
    return buf;
  }
  if (inner != 1 || nseg != 1 || ld < C) return buf;
  if (colsum_v4_ok(ld, C, in16)) {
    const ColsumPlan p = colsum_plan(ld, outer, 1, C, true, false);
    std::snprintf(buf, sizeof buf, "each %s rb=%lld chunk=%lld waves=%d", names[p.stage1], (long long)p.rb, (long long)p.chunk, p.waves);
    return buf;
  }
  const ColsumPlan p = colsum_plan(ld, outer, 1, C, false, true);
  std::snprintf(buf, sizeof buf, "%s rb=%lld chunk=%lld waves=%d launches=%d", names[p.stage1], (long long)p.rb, (long long)p.chunk,
                p.waves, (nbuf + COLSUM_BATCH_MAX - 1) / COLSUM_BATCH_MAX);
  return buf;
}

extern "C" int tecm_colsum(const float* in, int64_t ld, int64_t outer, int64_t inner, int32_t nseg, int32_t C,
                           float* out, int64_t ldo, int32_t accumulate, float scale, const TecmDrop* in_drop,
                           float* workspace, void* stream) {
  return colsum_impl(in, ld, outer, inner, nseg, C, out, ldo, accumulate, scale, in_drop, workspace, nullptr, 0, stream);
}

// The same pass also writes the (masked) values as a bf16 matrix twin[row][ld_twin]: the operand two bf16 contractions
// read next (their loaders would round the fp32 values to exactly these), at no extra read of `in`.
extern "C" int tecm_colsum_twin(const float* in, int64_t ld, int64_t outer, int64_t inner, int32_t nseg, int32_t C,
                                float* out, int64_t ldo, int32_t accumulate, float scale, const TecmDrop* in_drop,
                                float* workspace, void* twin_bf16, int64_t ld_twin, void* stream) {
  TECM_REQUIRE(twin_bf16 && ld_twin >= C && ld_twin % 4 == 0 && tecm_aligned(twin_bf16, 8), TECM_E_ARG,
               "tecm_colsum_twin: the bf16 twin needs 8-byte friendly rows of at least C values");
  return colsum_impl(in, ld, outer, inner, nseg, C, out, ldo, accumulate, scale, in_drop, workspace, twin_bf16, ld_twin, stream);
}

// out[i][c] = sum over rows of in[i][row*ld + c] for nbuf matrices of the same (rows, C) shape: the result of
// tecm_colsum(in[i], ld, rows, 1, 1, C, out[i], C, 0, 1.0f, NULL, ...) on each -- the same blocks, row chunks and order of
// every sum, bit for bit -- in one pair of launches for all of them (a grid dimension walks the pointer table, which
// travels in the kernel arguments).  Shapes the float4 first stage serves (C <= 1024) are reduced matrix by matrix.
extern "C" int tecm_colsum_batch(const float* const* in, float* const* out, int32_t nbuf, int64_t ld, int64_t rows, int32_t C,
                                 float* workspace, void* stream) {
  TECM_REQUIRE(in && out && workspace && nbuf > 0 && rows > 0 && C > 0 && ld >= C, TECM_E_ARG, "tecm_colsum_batch: bad arguments");
  for (int i = 0; i < nbuf; ++i) TECM_REQUIRE(in[i] && out[i], TECM_E_ARG, "tecm_colsum_batch: null matrix %d", i);
  bool any4 = false;                // would tecm_colsum take its float4 first stage for one of the matrices?
  for (int i = 0; i < nbuf; ++i) any4 = any4 || colsum_v4_ok(ld, C, tecm_aligned(in[i], 16) && tecm_aligned(workspace, 16));
  if (any4) {                       // then every matrix goes through tecm_colsum's own choice, one by one
    for (int i = 0; i < nbuf; ++i) {
      const int rc = colsum_impl(in[i], ld, rows, 1, 1, C, out[i], C, 0, 1.0f, nullptr, workspace, nullptr, 0, stream);
      if (rc != TECM_OK) return rc;
    }
    return TECM_OK;
  }
  const ColsumPlan p = colsum_plan(ld, rows, 1, C, false, true);       // as tecm_colsum's lane-per-column route with nseg = 1
  hipStream_t st = (hipStream_t)stream;
  for (int i0 = 0; i0 < nbuf; i0 += COLSUM_BATCH_MAX) {
    const int n = nbuf - i0 < COLSUM_BATCH_MAX ? nbuf - i0 : COLSUM_BATCH_MAX;
    ColsumBatch tab{};
    for (int i = 0; i < n; ++i) { tab.in[i] = in[i0 + i]; tab.out[i] = out[i0 + i]; }
    float* ws = workspace + (int64_t)i0 * p.rb * C;
    hipLaunchKernelGGL(colsum_stage1_batch, dim3(p.colblocks, (unsigned)p.rb, n), dim3(256), 0, st, tab, ld, rows, C, ws, p.chunk);
    TECM_CHECK_LAUNCH("tecm_colsum_batch/stage1");
    if (p.waves == 16)
      hipLaunchKernelGGL(colsum_stage2_batch<16>, dim3(p.colblocks, n), dim3(1024), 0, st, tab, ws, (int)p.rb, C);
    else
      hipLaunchKernelGGL(colsum_stage2_batch<8>, dim3(p.colblocks, n), dim3(512), 0, st, tab, ws, (int)p.rb, C);
    TECM_CHECK_LAUNCH("tecm_colsum_batch/stage2");
  }
  return TECM_OK;
}
