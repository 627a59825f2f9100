/*
 * tecmollm.h -- C ABI of libtecmollm_hip.so, the MI355X (gfx950) implementation of the
 * TEC-MoLLM forward/backward hot path.
 *
 * The reference (PANXIONG-CN/TEC-MoLLM) is 100 % Python and has no FFI of its own: its
 * hot path is `TEC_MoLLM.forward` (src/model/tec_mollm.py:59-125) calling torch /
 * torch_geometric / transformers / peft ops.  Each entry point below therefore cites the
 * reference *operation* it replaces; the Python-side mirror of the reference's module API
 * (tec-mollm_amd/src/model/{tec_mollm,modules}.py) binds these through ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless said otherwise;
 *   - the library never allocates or frees caller-visible memory (workspaces are passed in);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), no internal sync;
 *   - return value: 0 = launched, negative = TECM_E_* (nothing launched);
 *   - activation tensors after the spatial stage are "time-major": rows m = (b*T + t)*N + n,
 *     i.e. logical shape (B, T, N, C) with C contiguous -- see DESIGN.md "Data layout";
 *   - dropout masks are a pure function keep(seed, idx) (tecm_keep in csrc/common.h), so the
 *     backward pass recomputes them; idx = logical_row * ld + col of the tensor being dropped.
 */
#ifndef TECMOLLM_H
#define TECMOLLM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TECM_OK 0
#define TECM_E_ARG (-1)        /* bad shape / null pointer / unsupported size            */
#define TECM_E_ALIGN (-2)      /* pointer or leading dimension not aligned as required   */
#define TECM_E_LAUNCH (-3)     /* hipGetLastError() != hipSuccess after the launch       */
#define TECM_E_LDS (-4)        /* problem does not fit the 160 KiB LDS budget            */

#define TECM_ABI_VERSION 21
int tecm_abi_version(void);
/* Human-readable text for the last error on this thread (host pointer, never NULL). */
const char* tecm_last_error(void);

/* ------------------------------------------------------------------ temporal-window row view
 * A row view maps a logical row m = (bq*Lout + t_out)*N + n and an inner index kk = tap*Cw + c
 * onto a (B, Lin, N, ld) time-major tensor:
 *      t_in = t_out*stride_t + tap - pad ;  valid iff 0 <= t_in < Lin  (else the element is 0)
 *      addr = base + ((bq*Lin + t_in)*N + n)*ld + c
 * enabled == 0 means the plain view addr = base + m*ld + kk.
 * It expresses, without materialising anything: Conv1d im2col over time (modules.py:27),
 * the stride-2 1x1 conv (modules.py:36-41), einops 'b (p l) d -> b p (l d)' (modules.py:114)
 * and PredictionHead's view(batch, -1) (modules.py:307). */
typedef struct TecmWin {
  int32_t enabled;
  int32_t N;
  int32_t Lin, Lout;
  int32_t stride_t;
  int32_t taps;
  int32_t Cw;
  int32_t pad;
} TecmWin;

typedef struct TecmDrop {      /* keep-mask spec; p == 0 disables */
  float p;
  int32_t _pad;
  uint64_t seed;
  int64_t ld;                  /* idx = row*ld + col */
  /* NULL, or a device word ADDED to `seed` by the kernel when it starts: a training step whose launches were recorded
   * once (hipGraph) draws fresh masks at every replay by advancing that one word (tecm_seed_advance) -- the seeds in the
   * recorded kernel arguments never change.  The forward and the backward of a step read the same value. */
  const uint64_t* seed_dev;
} TecmDrop;

enum { TECM_A_MK = 0, TECM_A_KM = 1 };   /* A stored [m][k] (k contiguous) or [k][m] (m contiguous) */
enum { TECM_B_NK = 0, TECM_B_KN = 1 };   /* B stored [n][k] (k contiguous) or [k][n] (n contiguous) */
enum { TECM_ACT_NONE = 0, TECM_ACT_GELU_ERF = 1, TECM_ACT_GELU_TANH = 2 };

/* fp32 GEMM on exact-f32 MFMA (v_mfma_f32_32x32x2_f32):  C = epilogue(alpha * A_view . B_view).
 * Replaces every dense contraction on the path: nn.Conv1d (modules.py:27,36), nn.Linear
 * (modules.py:98,287,290), transformers Conv1D c_attn/c_proj/c_fc (pytorch_utils.py:95-121 via
 * modules.py:208), peft LoRA A/B (modules.py:177-186), GATv2 is NOT here (tecm_spatial_*), and
 * their autograd backward (dX and dW forms).
 * Epilogue order: v = alpha*acc; v += bias[n]; v += rowbias[((m / rb_div) % rb_mod)*rb_ld + n];
 *   if preact: preact[m*ldp+n] = v   (a bf16 preact stores bf16(v) and continues with v = float(bf16(v)));
 *   if dact_src: v *= act'(dact_src[m*ldd+n])   else: v = act(v)      -- one or the other, never both: with dact_src,
 *     `act` only names the activation whose derivative is taken and must not be TECM_ACT_NONE (TECM_E_ARG);
 *   v = dropout(v, out_drop): mask index row*out_drop.ld + col of the element of C being stored (under c_win the
 *     target row and column of the view);
 *   if residual: v += residual[m*ldr+n];  if accumulate: v += the previous value of the element of C being stored;
 *   store C (through c_win when enabled: column n is the inner index kk of the view; an element whose t_in falls
 *   outside [0, Lin) is dropped).  split_k > 1 applies the same epilogue to the reduced sum.
 * tests/gemm_epilogue_ref.py states this order in fp64; tests/test_gpu_gemm_epilogue.py holds every kernel family to it. */
/* io_bf16 (tecm_gemm_bf16 only, 0 everywhere else): which tensors of the call already are / shall be bf16 in HBM.
 * A bf16 operand has its leading dimension counted in bf16 elements (multiple of 8, 16-byte aligned base) and a contiguous
 * extent that is a multiple of 8: K for [row][k] storage, M for A stored [k][m], N for B stored [k][n]; a window view of it
 * needs Cw % 8 == 0 (TECM_E_ALIGN / TECM_E_ARG otherwise).  Served: MK x NK with plain views -- A, B or both; MK x NK behind
 * a window -- A alone behind a_win (both only where the LDS-DMA kernels take the view: pad-free taps of whole K-tiles);
 * MK x KN -- A alone; KM x KN -- A, B or both.  An fp32 partner needs the float4 loader (16-byte aligned, leading dimension,
 * and K where k is contiguous, multiples of 4); every other combination is TECM_E_ARG.  tests/test_gpu_gemm_shapes.py
 * holds each of these to the contract either side of its tile edges and asserts the refusals.
 * TECM_IO_C_BF16 writes C as bf16
 * (ldc in bf16 elements; needs the float4-friendly epilogue, no residual / accumulate / c_win / split_k); preact,
 * dact_src, bias stay fp32.  Rounding an activation once where it is produced instead of at every consumer's
 * loader gives bit-identical results at half the bytes.
 * TECM_IO_PRE_BF16: `preact` and `dact_src` are bf16 tensors (ldp / ldd in bf16 elements, multiples of 4, 8-byte
 * aligned; float4-friendly epilogue, tanh-GELU only, no split_k).  The value is rounded to bf16 BEFORE the
 * activation -- the store is `preact = bf16(v); v = act(float(preact))` -- so the forward's act() and the
 * backward's act'() are evaluated at the same point: what torch.autocast does to the output of a Linear that
 * feeds an activation (train.py:68), and what the bf16-emulating oracle (oracle/ref_cpu.BF16) restates. */
#define TECM_IO_A_BF16 1
#define TECM_IO_B_BF16 2
#define TECM_IO_C_BF16 4
#define TECM_IO_PRE_BF16 8
typedef struct TecmGemm {
  int64_t M, N, K;
  const float* A; int64_t lda; int32_t a_layout; int32_t io_bf16; TecmWin a_win; TecmDrop a_drop;
  const float* B; int64_t ldb; int32_t b_layout; int32_t _p1; TecmWin b_win; TecmDrop b_drop;
  float* C; int64_t ldc; TecmWin c_win;
  float alpha; int32_t act;
  const float* bias;
  const float* rowbias; int64_t rb_ld; int32_t rb_div; int32_t rb_mod;
  float* preact; int64_t ldp;
  const float* dact_src; int64_t ldd;
  TecmDrop out_drop;
  const float* residual; int64_t ldr;
  int32_t accumulate;
  int32_t split_k;             /* >1: partial sums go to workspace[split][M][N], then reduced */
  float* workspace;            /* >= split_k*M*N floats when split_k > 1 */
  /* Two optional HINTS (all zero: none).  They promise something about the caller's data; a kernel family may ignore
   * either (ignoring is always correct), tecm_gemm_f32 honours them where stated and tecm_gemm_last_skipped_flops says
   * what a call left out.  Both rectangles are periodic in the row: rows with row % period < rows, period > 0.  Both are
   * honoured only by the plain float4 instances: split_k <= 1, 16-byte friendly operands, no a_win / b_win, no a_drop / b_drop.
   * Dead output rectangle: the elements of C with row % dead_period < dead_rows and col < dead_cols will never be read.
   *   A block tile whose rows inside M and whose columns inside N all lie in the rectangle is not computed and NOTHING is
   *   stored for it (C keeps its previous contents there); tiles on the rectangle's edge are computed whole.  Also
   *   needs: no c_win, no preact, no TECM_ACT_GELU_ERF (passes that walk all of C or write a second output).
   * Known-zero A rectangle: A[row][k] is +0 or -0 for row % zero_period < zero_rows and k < zero_k (zero_k a multiple of
   *   32, below K).  A block tile whose rows inside M all lie in the rectangle starts its K loop at zero_k: the accumulators
   *   start at +0 and fma(+-0, b, +0) = +0 for finite b, so the result is bit for bit that of the full loop (a non-finite B
   *   element against such a zero gives NaN in the full loop and is not seen here).  Also needs A stored [m][k]. */
  int32_t dead_period, dead_rows, dead_cols;
  int32_t zero_period, zero_rows, zero_k;
} TecmGemm;
int tecm_gemm_f32(const TecmGemm* desc, void* stream);
/* Same contract on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16): operands are rounded to bf16 (RNE) while
 * staged into LDS, accumulation / epilogue / outputs stay fp32 -- what torch.autocast(bf16) does to the inputs
 * of Linear / Conv1d / Conv1D (train.py:68).  Operands must be 16-byte friendly (else TECM_E_ALIGN). */
int tecm_gemm_bf16(const TecmGemm* desc, void* stream);
/* "bf16x3": fp32 tensors, every factor split into a bf16 head and a bf16 remainder while it is staged, each product
 * evaluated as lo.hi + hi.lo + hi.hi on the bf16 matrix cores with fp32 accumulation (~16 mantissa bits per factor,
 * dot-product relative error ~1e-5; the bf16 MFMA runs at 16x the exact-f32 MFMA rate on gfx950).  Opt-in
 * (model_config["precision"] = "bf16x3"); serves the plain MK x NK contraction only, TECM_E_ARG otherwise. */
int tecm_gemm_bf16x3(const TecmGemm* g, void* stream);
/* "bf16x6": three-way split (hi + mid + lo carries all 24 mantissa bits), six products hi.lo + lo.hi + mid.mid +
 * hi.mid + mid.hi + hi.hi: only terms below 2^-24 of a product are dropped -- fp32-grade accuracy at 6/16 of the exact
 * matrix time.  Same scope and return convention as tecm_gemm_bf16x3. */
int tecm_gemm_bf16x6(const TecmGemm* g, void* stream);

/* Weight gradients in bf16 mode (a_layout KM x b_layout KN, both operands bf16 tensors, split_k >= 2: the backward of
 * every trainable nn.Linear / Conv1d(k=1) / LoRA matrix of the path, reference train.py:85) are served inside
 * tecm_gemm_bf16 by a natural-orientation LDS-DMA kernel (csrc/gemm_bf16_tn.hip) for the output shapes it is built for.
 * This returns the split count that kernel wants for an M x N output contracted over K rows (one or two rounds of
 * blocks on 256 CUs, slabs kept under a tenth of the operand bytes), or 0 when the shape is not served -- the caller
 * sizes split_k / the workspace with it; any split_k >= 2 is accepted.  Pure host function. */
int32_t tecm_gemm_tn_splits(int64_t M, int64_t N, int64_t K);
/* Rows per wave row (half the tile height: 128, 112 or 96) the eight-phase bf16 GEMM inside tecm_gemm_bf16 uses for an
 * M x N result on this device: the height whose tile count wastes least of the last round of CUs (csrc/gemm_bf16_p8.hip).
 * Exposed so that a caller's per-kernel accounting can name the instantiation a call runs on. */
int tecm_p8_rows(int64_t M, int64_t N);
/* The block -> tile map the bf16 and split-bf16 GEMM kernels apply to blockIdx.x (csrc/gemm_tile_map.h, compiled here for
 * the host; the fp32 kernel carries the same formula inline): block `id` of a tiles_m x tiles_n grid whose L2 super-tiles
 * are group_m m-tiles tall computes tile (*tm, *tn).  Exposed so that a host test can check the map is a bijection.  Pure
 * host function. */
void tecm_gemm_tile_of_block(int id, int tiles_m, int tiles_n, int group_m, int* tm, int* tn);
/* The same for every id in 0 .. tiles_m * tiles_n - 1 in one call: tm[id], tn[id]. */
void tecm_gemm_tiles_of_blocks(int tiles_m, int tiles_n, int group_m, int* tm, int* tn);
/* The row test behind both hints of TecmGemm, as the kernels apply it to a block tile: 1 when every row r of [r0, r1) has
 * r % period < rows (period > 0, 0 <= r0 < r1), else 0.  Pure host function (csrc/gemm_tile_map.h compiled for the host). */
int tecm_gemm_rows_in_rect(int64_t r0, int64_t r1, int32_t period, int32_t rows);
/* Number of bm x bn block tiles of an M x N matrix that lie wholly inside the periodic rectangle (row % period < rows,
 * col < cols), counting only a tile's rows inside M and columns inside N: the tiles the dead-rectangle hint skips
 * (cols = dead_cols) and, with cols = N and bn = N, the row tiles the zero-rectangle hint shortens.  Pure host function. */
int64_t tecm_gemm_rect_tiles(int64_t M, int64_t N, int32_t bm, int32_t bn, int32_t period, int32_t rows, int64_t cols);
/* 2 * (multiply-adds) this thread's most recent successful tecm_gemm_* call did NOT issue because it honoured a hint of its
 * descriptor: over the skipped tiles rows x cols x K, over the shortened ones rows x cols x zero_k, rows and columns counted
 * inside M and N -- the part of 2 * M * N * K that was not computed.  0 when the call's kernel ignored the hints or none was set.  Pure host function. */
int64_t tecm_gemm_last_skipped_flops(void);
/* Name of the contraction kernel (template arguments included, e.g. "gemm_kernel<0,0,4,4,128,false,false,128>") that this
 * thread's most recent successful tecm_gemm_* call launched; the split-K reducer and the erf-GELU pass behind it are not
 * reported.  "" before the first call, unspecified after a failed one.  Host pointer, valid for the life of the library.
 * Pure host function. */
const char* tecm_gemm_last_kernel(void);

/* ------------------------------------------------------------------ stage a-1..a-3 (fused)
 * SpatioTemporalEmbedding.forward (modules.py:230-266) + GATv2Conv (modules.py:329-336,:356)
 * + residual (tec_mollm.py:94).  The two permute copies (tec_mollm.py:84, :100-106) disappear:
 * input and output both stay (B, L, N, *) time-major. */
typedef struct TecmSpatial {
  int32_t B, L, N, Cin, Demb, H;          /* C = Cin + Demb = H*Ch */
  int32_t graphs_with_edges;              /* R: graphs g = t*B + b < R aggregate neighbours;
                                             1 = the reference's literal behaviour, B*L = every timestep */
  int32_t num_tiles, tile_nodes, win_max; /* node tiling computed by the host from the CSR */
  const float* x;                         /* (B, L, N, Cin) contiguous */
  const float* tf; int64_t tf_sb, tf_sl, tf_sn, tf_sf;   /* (B,L,N,4) with element strides; sn may be 0 */
  const float* node_tab; const float* tod_tab; const float* doy_tab; const float* year_tab;
  const float* season_tab;                /* (rows, Demb) each */
  int32_t year_rows;
  int32_t tile_edges_max;                 /* max over tiles of rowptr[n1] - rowptr[n0] (CSR slice staged in LDS) */
  const float* Wl; const float* bl; const float* Wr; const float* br;   /* (C,C),(C) */
  const float* att;                       /* (H, Ch) */
  const float* bias;                      /* (C) */
  const int32_t* rowptr;                  /* (N+1) CSR by target, self loops removed */
  const int32_t* colidx;                  /* (E) source node ids */
  const int32_t* tile_lo; const int32_t* tile_hi;   /* (num_tiles) window [lo,hi) of sources u targets */
  TecmDrop alpha_drop;                    /* GATv2 dropout on attention coefficients (modules.py:333) */
  float* out;                             /* (B, L, N, C) */
  /* Device error word (one int32, never NULL, owned by the caller, sticky: the kernels only OR bits in).  The
   * reference's nn.Embedding lookups raise on an out-of-range index (modules.py:255-258); here an index outside its
   * table sets TECM_BAD_TOD/DOY/YEAR/SEASON, and every output row built from it is NaN -- never a clamped, valid
   * looking embedding.  The caller reads the word back when it next synchronises (tecmollm/devcheck.py). */
  int32_t* err_flag;
  int32_t flags;                          /* TECM_SPATIAL_*; 0 = the fused stage as TEC_MoLLM.forward runs it */
  int32_t out_ld;                         /* row pitch of out: 24 (padded, 16-byte rows) in the fused path, >= 22 otherwise */
} TecmSpatial;
/* Stand-alone forms of the two modules the kernel fuses (their own `forward` in the reference):
 *   TECM_SPATIAL_EMBED_ONLY   SpatioTemporalEmbedding.forward (modules.py:230-266): out = cat([x, emb]), no graph work;
 *   TECM_SPATIAL_NO_RESIDUAL  SpatialEncoder.forward (modules.py:340-359): out = GATv2Conv(h) without `h +`; with
 *                             Demb = 0 the input rows ARE h (Cin = 22) and no table is read. */
#define TECM_SPATIAL_EMBED_ONLY 1
#define TECM_SPATIAL_NO_RESIDUAL 2
#define TECM_BAD_TOD 1
#define TECM_BAD_DOY 2
#define TECM_BAD_YEAR 4
#define TECM_BAD_SEASON 8
int tecm_spatial_fwd(const TecmSpatial* d, void* stream);
/* The same stage in a second formulation for the configuration TEC_MoLLM.forward runs (tec_mollm.py:84-94 with the
 * block-uniform time features of train.py:65, flags == 0, out_ld == 24, Cin 6 or 10): one 256-thread block per (tile,
 * graph) item, 37 KiB of LDS, four blocks per CU; the input transforms split into a graph-independent node part, a
 * per-graph vector (both computed by a set-up launch into `ws`) and a Cin-wide per-row part (csrc/spatial_fwd2.hip).
 * tecm_spatial_fwd2_ws_floats: floats of workspace the call needs, or 0 when this formulation does not serve `d` (then
 * use tecm_spatial_fwd).  Results agree with tecm_spatial_fwd to fp32 summation order. */
int64_t tecm_spatial_fwd2_ws_floats(const TecmSpatial* d);
int tecm_spatial_fwd2(const TecmSpatial* d, float* ws, void* stream);

typedef struct TecmSpatialGrads {
  const float* dout;                      /* (B, L, N, C) */
  float* d_node_tab;                      /* (N, Demb)  accumulated with float atomics: zero before call */
  float* d_tod_tab; float* d_doy_tab; float* d_year_tab; float* d_season_tab;   /* atomics: zero before call */
  float* partials; int64_t partial_ld;    /* (num_blocks, partial_ld) per-block sums of
                                             [dWl(C*C) dbl(C) dWr(C*C) dbr(C) datt(C) dbias(C)] */
  int32_t t_chunk; int32_t num_blocks;    /* num_blocks = tecm_spatial_bwd_blocks(d): the grid the library launches
                                             (persistent blocks over contiguous (tile, graph) ranges); t_chunk unused */
  /* the tile's edges grouped by SOURCE (d x_l is gathered per source row, no atomics): for tile k with window
   * [lo, hi) and edge segment [rowptr[n0], rowptr[n1]) of the by-target CSR,
   *   src_ptr[src_ptr_off[k] + w] .. src_ptr[src_ptr_off[k] + w + 1]   (w = j - lo, 0 <= w < hi - lo)
   * index, relative to rowptr[n0], the entries of src_col that leave source j; an entry is
   * ((target - n0) << 16) | pos, pos = position of the edge inside the tile's by-target segment (e - rowptr[n0]). */
  const int32_t* src_ptr; const int32_t* src_col; const int32_t* src_ptr_off;
} TecmSpatialGrads;
int tecm_spatial_bwd(const TecmSpatial* d, const TecmSpatialGrads* g, void* stream);
/* The same backward in the second formulation (csrc/spatial_bwd2.hip) for the configuration tecm_spatial_fwd2 serves: blocks
 * of 256 threads over (tile, chunk of graphs), ~45 KiB of LDS, three per CU.  Same TecmSpatialGrads contract (tables by
 * atomics into zeroed buffers, one row of `partials` per block in the same column layout) with
 * num_blocks = tecm_spatial_bwd2_blocks(d) (0 = not served: use tecm_spatial_bwd) and a workspace of
 * tecm_spatial_fwd2_ws_floats(d) floats that the call fills itself. */
int tecm_spatial_bwd2_blocks(const TecmSpatial* d);
int tecm_spatial_bwd2(const TecmSpatial* d, const TecmSpatialGrads* g, float* ws, void* stream);
/* Number of blocks (= rows of TecmSpatialGrads.partials) tecm_spatial_bwd will launch for `d`; negative = TECM_E_*. */
int tecm_spatial_bwd_blocks(const TecmSpatial* d);
/* Dynamic LDS bytes tecm_spatial_fwd / tecm_spatial_bwd need for a tiling (TecmSpatial::win_max, tile_nodes, tile_edges_max,
 * Demb); the launchers refuse with TECM_E_LDS above 160 KiB, so a caller picks its tile size with these.  Pure host functions. */
int64_t tecm_spatial_fwd_lds_bytes(int32_t win_max, int32_t tile_nodes, int32_t tile_edges_max);
int64_t tecm_spatial_bwd_lds_bytes(int32_t win_max, int32_t tile_nodes, int32_t tile_edges_max, int32_t Demb);

/* Gradient of the fused stage (flags == 0, Cin 6 or 10) with respect to its input x (csrc/spatial_dx.hip):
 *   dx_n = dout_n[:Cin] + W_l[:, :Cin]^T d x_l[n] + W_r[:, :Cin]^T d x_r[n]
 * for the same descriptor the forward ran with (alpha_drop included: the masks are recomputed).  No float atomics: dx is
 * bit-reproducible.  Any graph the forward accepts is served, with block-uniform or per-node time features; the tiling
 * fields of `d` are checked but not used.  A time index outside its table gives NaN rows of dx and sets *err_flag. */
typedef struct TecmSpatialDx {
  const float* dout;                      /* (B, L, N, 24): the padded rows the fused stage writes, 16-byte aligned */
  float* dx; int64_t dx_ld;               /* (B*L*N, dx_ld >= Cin): columns [0, Cin) of every row are written */
  float* ws;                              /* tecm_spatial_dx_ws_floats(d) floats, 16-byte aligned; contents undefined after */
  /* the whole graph's non-self edges grouped by SOURCE: entries src_rowptr[j] .. src_rowptr[j + 1] leave node j; entry q
   * goes to target src_target[q] and is slot src_slot[q] of that target's list in the by-target CSR
   * (colidx[rowptr[target] + slot] == j), which makes its dropout index the forward's. */
  const int32_t* src_rowptr;              /* (N+1) */
  const int32_t* src_target;              /* (E) */
  const int32_t* src_slot;                /* (E) */
} TecmSpatialDx;
/* Floats of workspace the call needs (x_l, x_r and three softmax statistics per (row, head) for one chunk of graphs, at most
 * 64 MiB unless a single graph needs more), or 0 when `d` is not served.  Pure host function. */
int64_t tecm_spatial_dx_ws_floats(const TecmSpatial* d);
int tecm_spatial_dx(const TecmSpatial* d, const TecmSpatialDx* g, void* stream);

/* The GATv2 attention coefficients of the same stage (csrc/spatial_attn.hip): what PyG's GATv2Conv returns for
 * return_attention_weights=True at the reference's call site (modules.py:329-336,:356), before the attention dropout:
 *   alpha_ij = exp(e_ij - max_j e_ij) / (sum_j exp(e_ij - max) + 1e-16),  e_ij = att_k . lrelu(x_l[j,k] + x_r[i,k])
 * over the in-edges j of target i plus its self loop, per head, per graph.  It takes the descriptor the forward ran with: the
 * fused stage (flags == 0, Cin 6 or 10, Demb = 22 - Cin) or the stand-alone GATv2 (TECM_SPATIAL_NO_RESIDUAL, Cin = 22,
 * Demb = 0); the tiling fields of `d` are checked but not used, alpha_drop is ignored, `out` is not written.
 * Entries of a graph in KERNEL ORDER: the by-target CSR entries q in [0, E) in rowptr / colidx order, then the N self loops
 * at E + i; E2 = E + N.  A graph g = t*B + b >= graphs_with_edges holds its self loops only: alpha = 1 there, 0 in every
 * CSR entry, entropy 0, all exact.  A time index outside its table gives NaN coefficients in the graph's rows that read it
 * and sets TECM_BAD_* in *d->err_flag.
 *   raw export    alpha (B*L, E2, H) floats, graphs in memory order gm = b*L + t: entry q of graph gm, head h, is written at
 *                 alpha[(gm*E2 + p(q))*H + h] with p(q) = perm[q] for a CSR entry (perm NULL: q) and p(E + i) = E + i.  With
 *                 perm = the position of every CSR entry in the caller's edge list the export is in PyG's order: the
 *                 non-self edges as given, then the self loops.  A perm value outside [0, E2) drops that entry.
 *   accumulation  edge_stats (G, 3, E2, H) doubles in kernel order: sum alpha, sum alpha^2, sum m with the message size
 *                 m_ij = alpha_ij * |x_l[j, head]|_2;  node_stats (G, N, H) doubles: sum of the entropy -sum_j alpha ln alpha
 *                 of target i;  counts (G) int64: graphs added.  group (B*L) int32 in memory order names the group of every
 *                 graph (NULL: group 0); an id outside [0, num_groups) skips the graph and sets TECM_BAD_GROUP in
 *                 *d->err_flag, never clamped.  TECM_ATTN_SKIP_UNCONNECTED leaves the graphs without edges out of every sum.
 *                 Every cell has ONE owning thread, which adds the graphs of the call in ascending gm with plain loads and
 *                 stores: no atomics, so the same calls in the same order give the same bits, whatever the workspace size.
 * Either part may be left out (alpha NULL / edge_stats NULL), not both.
 * ws: the call walks chunks of graphs through it (x_l, x_r as 24-float rows; alpha, m and the entropy of the chunk when
 * accumulating).  ws_floats = floats it holds, 0 = tecm_spatial_attention_ws_floats(d, a), which is at most 64 MiB unless one
 * graph needs more; any size that holds one graph is accepted (smaller: more chunks, same bits). */
#define TECM_ATTN_SKIP_UNCONNECTED 1
typedef struct TecmSpatialAttn {
  float* alpha;                           /* (B*L, E2, H) or NULL */
  const int32_t* perm;                    /* (E) or NULL = identity */
  double* edge_stats;                     /* (G, 3, E2, H) or NULL = no accumulation */
  double* node_stats;                     /* (G, N, H) */
  int64_t* counts;                        /* (G) */
  const int32_t* group;                   /* (B*L) or NULL */
  float* ws; int64_t ws_floats;           /* 16-byte aligned; contents undefined after */
  int32_t num_groups;                     /* G */
  int32_t E;                              /* entries of the by-target CSR: rowptr[N] */
  int32_t flags;                          /* TECM_ATTN_* */
  int32_t _pad;
} TecmSpatialAttn;
/* Floats of workspace the call asks for by default, or 0 when (d, a) is not served.  Pure host function. */
int64_t tecm_spatial_attention_ws_floats(const TecmSpatial* d, const TecmSpatialAttn* a);
int tecm_spatial_attention(const TecmSpatial* d, const TecmSpatialAttn* a, void* stream);

/* ------------------------------------------------------------------ stage a-4 normalisation
 * nn.GroupNorm(1, C) + nn.GELU() (modules.py:28-29) for the three parallel branches at once.
 * y/act: (B, L, N, CT) time-major with CT = 3*Cout (branch j owns channels [j*Cout,(j+1)*Cout)).
 * stats: (B*N, 3, 2) = mean, rstd per sequence and branch. */
/* io_bf16 (BASELINE configs[2] only, 0 otherwise): TECM_GN_OUT_BF16 -- act (forward) / dy (backward) is written as bf16:
 * its only readers are bf16 matrix-core GEMMs that would round it in their loaders (train.py:68 autocast semantics).
 * y, the statistics and all arithmetic stay fp32. */
#define TECM_GN_OUT_BF16 2
/* backward only, with TECM_GN_OUT_BF16: dact is a bf16 tensor (written by the bf16 GEMM of the strided 1x1 conv's d-input) */
#define TECM_GN_DACT_BF16 4
/* y itself is the bf16 tensor a bf16 Conv1d hands to the fp32 GroupNorm under autocast (train.py:68; tecm_conv_fwd_bf16 with
 * y_bf16): forward with TECM_GN_OUT_BF16, backward with TECM_GN_OUT_BF16 | TECM_GN_DACT_BF16 -- every tensor bf16, statistics
 * and arithmetic fp32.  Served for L * 3*Cout/8 <= 2304 (tecm_gn_y16_supported). */
#define TECM_GN_Y_BF16 1
/* forward only, with TECM_GN_Y_BF16 | TECM_GN_OUT_BF16: `stats` is an INPUT -- the (mean, rstd) tecm_conv_fwd_bf16 computed from
 * the rounded y it produced (TecmConvFwd::stats); the norm + GELU then is elementwise over the time steps act keeps. */
#define TECM_GN_STATS_GIVEN 8
int tecm_gn_y16_supported(int32_t L, int32_t N, int32_t Cout);
/* 1 when BOTH directions have a register-resident kernel (the only fp32-y kernels that take a bf16 act / dact / dy, and the
 * only ones that serve act_stride > 1): L * 3*Cout/4 quads in whole rounds of 4 or 8 waves, at most 9 per lane.  Pure host
 * function. */
int tecm_gn_reg_supported(int32_t L, int32_t N, int32_t Cout);
/* The kernel tecm_groupnorm_gelu_fwd / _bwd launches for these arguments and 16-byte aligned tensors, with its template
 * arguments -- "gn_gelu_fwd_reg<1,4,9,false>", "gn_bwd_sums16_kernel<2>+gn_bwd_apply16_kernel<2>" -- or "" where the
 * launcher refuses.  has_seq_sums: the backward call passes a seq_sums workspace.  The answers come from the functions the
 * launchers route by (the environment switches TECM_GN_BWD_SPLIT / TECM_GN_BWD_WPS included).  Pure host functions; the
 * string lives until this thread's next call of either. */
const char* tecm_gn_fwd_path(int32_t L, int32_t N, int32_t Cout, int32_t io_bf16, int32_t act_stride);
const char* tecm_gn_bwd_path(int32_t L, int32_t N, int32_t Cout, int32_t io_bf16, int32_t has_seq_sums);
/* act_stride s >= 1: only the time steps t % s == 0 are written, into a COMPACT (B, ceil(L / s), N, CT) tensor -- the
 * stride-s 1x1 conv behind the block (modules.py:36-41) reads nothing else; the statistics cover every step.  s > 1 is
 * served by the register-resident kernels only (TECM_E_ARG otherwise: callers ask tecm_gn_reg_supported first). */
int tecm_groupnorm_gelu_fwd(const void* y, const float* gamma, const float* beta, void* act,
                            float* stats, int32_t B, int32_t L, int32_t N, int32_t Cout, float eps,
                            int32_t io_bf16, int32_t act_stride, void* stream);
/* dact is (B, L/dstride, N, CT): the gradient exists only at t % dstride == 0 (stride-s 1x1 conv).
 * dgb_partials: (num_blocks, 3*CT) per-block [dgamma | dbeta | column sums of dy] -- the last third is the
 * gradient of the Conv1d biases in front of the norm (modules.py:27), free here since dy is being written;
 * returns num_blocks via *num_blocks when dy == NULL (query mode, nothing launched). */
int tecm_groupnorm_gelu_bwd(const void* dact, int32_t dstride, const void* y, const float* gamma,
                            const float* beta, const float* stats, void* dy, float* dgb_partials,
                            int32_t* num_blocks, int32_t B, int32_t L, int32_t N, int32_t Cout,
                            int32_t io_bf16,
                            float* seq_sums /* optional workspace of B*N*6 floats (all-bf16 form, Cout 64 / 128): the backward
                                               then runs as two streaming kernels -- per-sequence sums, then an elementwise
                                               pass -- instead of holding each sequence in registers.  NULL: one kernel */,
                            void* stream);

/* ------------------------------------------------------------------ stage a-6 pieces
 * nn.LayerNorm(768, eps=1e-5) of GPT2Block / ln_f (modeling_gpt2.py:262-310, :620). */
/* y (fp32) and / or y16 (bf16, RNE): the bf16 copy feeds a bf16 matrix-core GEMM (BASELINE configs[2]) that would
 * round the fp32 value in its loader anyway -- same bits, half the bytes; either pointer may be NULL, not both. */
int tecm_layernorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, float* y,
                       int64_t ldy, void* y16, int64_t ldy16,
                       void* y16d /* optional third output: bf16(dropout(y, drop)) -- the LoRA branch's input, peft
                                     lora_dropout in front of lora_A (modules.py:181), cast as autocast casts it */,
                       int64_t ldy16d, const TecmDrop* drop /* of y16d; element index row*drop->ld + c; p = 0: no mask */,
                       int32_t y16d_seq_T, int32_t y16d_seq_N /* both > 0: y16d is written SEQUENCE-major -- the time-major
                                     row (b, t, n) of M = B*T*N goes to row (b, n, t): PredictionHead's view(batch, -1)
                                     (modules.py:307) of ln_f's output as a plain [B*N][T*D] matrix.  0, 0: same rows as y */,
                       int32_t y16d_f32 /* != 0: y16d is an fp32 matrix (16-byte aligned), dropout(y, drop) unrounded: the
                                     fp32 head operand -- the values tecm_dropout_apply makes of y, bit for bit */,
                       float* stats /* (M,2) mean,rstd */, int64_t M, int32_t D, float eps, void* stream);
/* dx = dres (optional) + LN'(dy).  Optional second output dx_masked = dropout(dx, mask_drop): the
 * residual-stream gradient is consumed twice in GPT2Block's backward, once as is (residual path) and
 * once through the resid dropout in front of a GEMM; emitting the masked copy here costs one extra
 * store instead of one hash per element per GEMM column tile.  dgb_partials (num_blocks, 2*D);
 * dx == NULL only queries *num_blocks. */
/* masked_bf16 != 0: dx_masked is a bf16 (M, D) matrix (its only reader is a bf16 GEMM). */
/* Optional second gradient stream of the same tensor, added before the LayerNorm backward:
 *   dy[row][c] += keep(row*drop.ld + c) / (1 - p) * dy2[row][c]        (drop.p == 0: no mask)
 * -- the gradient peft's LoRA branch returns for its input (lora_A's d-input GEMM, modules.py:177-186) reaching the
 * LayerNorm output through lora_dropout's backward (modules.py:181).  dy2: (M, D) fp32 or bf16 with leading dimension ld. */
typedef struct TecmLnAdd {
  const void* dy2;
  int64_t ld;
  int32_t bf16, _pad;
  TecmDrop drop;
} TecmLnAdd;
/* dy in the sequence-major form tecm_layernorm_fwd can write y16d in (rows (b, n, t), bf16 or fp32) and still in front of the
 * forward's dropout:  dy[(b,t,n)][c] = keep((b,t,n), c) / (1 - p) * dy16[(b,n,t)][c]  -- the gradient the head's first Linear
 * returns for F.dropout(ln_f(h)) (tec_mollm.py:115), taken as it is.  T == 0 / NULL: plain rows. */
typedef struct TecmLnDyMap {
  int32_t T, N;
  TecmDrop drop;                 /* p == 0: no mask */
} TecmLnDyMap;
int tecm_layernorm_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma,
                       const float* stats, const float* dres, float* dx, void* dx_masked, int32_t masked_bf16,
                       const TecmDrop* mask_drop, float* dgb_partials, int32_t* num_blocks, int64_t M, int32_t D,
                       const TecmLnAdd* add /* NULL: none */,
                       int32_t dy_bf16 /* != 0: dy is bf16 -- the gradient a bf16 Linear returns for its input under
                                          autocast (train.py:68) */,
                       const TecmLnDyMap* dymap /* NULL: none; dy bf16 or fp32, no second stream */,
                       int32_t skip_dx /* != 0: the unmasked dx has no reader -- its store is left out and the dx buffer is not
                                          touched (still non-NULL: NULL queries); needs dx_masked */,
                       void* stream);

/* Causal multi-head self-attention over T tokens per sequence (GPT2Attention, modeling_gpt2.py:54-73,
 * :144-226; all-ones attention_mask tec_mollm.py:111 => pure causal).  qkv: (B,T,N,3*D) time-major
 * rows, ctx: (B,T,N,D).  head_dim = D/heads must be 64.  1 <= T <= 1024 (GPT-2's positions; T > 32 runs the matrix-core
 * kernels of attention_long.hip, same layout and results contract).  Dropout on the probabilities, 64-bit index
 * (((b*N + n)*heads + h)*T + i)*T + j. */
/* io_bf16: TECM_ATT_OUT_BF16 -- ctx is a bf16 (B,T,N,D) tensor (its only reader, attn.c_proj, is a bf16 GEMM);
 * TECM_ATT_QKV_BF16 -- qkv is a bf16 (B,T,N,3*D) tensor (bf16 mode: the c_attn GEMM stores its output as bf16, which is
 * what a Linear's output is under torch.autocast, train.py:68; scores, softmax and the weighted sum stay fp32). */
#define TECM_ATT_OUT_BF16 1
#define TECM_ATT_QKV_BF16 2
#define TECM_ATT_DCTX_BF16 4     /* backward only, with TECM_ATT_QKV_BF16: dctx is the bf16 tensor attn.c_proj's d-input GEMM wrote */
int tecm_attention_fwd(const float* qkv, void* ctx, int32_t io_bf16, int32_t B, int32_t T, int32_t N, int32_t heads,
                       int32_t D, const TecmDrop* prob_drop, void* stream);
/* io_bf16: TECM_ATT_OUT_BF16 -- dqkv is a bf16 (B,T,N,3*D) tensor (its readers, the c_attn dX and the LoRA-B dW GEMMs, are
 * bf16 GEMMs); TECM_ATT_QKV_BF16 -- qkv is the bf16 tensor the forward read; TECM_ATT_DCTX_BF16 -- dctx is bf16 (else fp32). */
int tecm_attention_bwd(const float* qkv, const float* dctx, void* dqkv, int32_t io_bf16, int32_t B, int32_t T, int32_t N,
                       int32_t heads, int32_t D, const TecmDrop* prob_drop, void* stream);
/* Query 0 of a causal sequence sees one key: its softmax is 1 whatever q_0 . k_0 is, and its score gradient is 0.  The
 * kernels with a compile-time T (T = 1, 2, 3, 4, 6, 8, 12) use that: neither the forward nor the backward loads the q
 * columns of a token-0 row, and the backward writes dq_0 = +0.  (Bit for bit the full arithmetic for finite inputs; a
 * non-finite q_0 . k_0, which makes the reference NaN, is not seen.)  Returns 0 for such a T -- the caller may then leave
 * those 64 * heads columns of the token-0 rows unwritten (TecmGemm's dead-rectangle hint) and rely on dq_0 = 0 (its
 * zero-rectangle hint) -- and 1 for every other T the entry points accept.  Pure host function. */
int tecm_attention_reads_q0(int32_t T);

/* The causal attention probabilities of one GPT-2 block, handed to the caller (csrc/attention_probs.hip): what Hugging Face's
 * GPT2Attention returns for output_attentions=True (modeling_gpt2.py:144-226) at the reference's call site
 * (LLMBackbone.forward, modules.py:205-209), BEFORE the attention dropout -- what eval() uses and what training draws its
 * masks over.  The production kernels (tecm_attention_fwd) form them in registers and keep only ctx.
 *   p_ij = exp(s_ij - max_j s_ij) / sum_{j<=i} exp(s_ij - max),   s_ij = (q_i . k_j) / 8,   all fp32;
 * the denominator is the fp32 sum of exactly the i + 1 numerators that are then divided (no online rescaling), so a row sums
 * to 1 within (i + 2) * 2^-24.  Row 0 is [1, 0, ...] by definition: the q columns of the token-0 rows are NEVER read, at any
 * T (in fp32 mode the c_attn GEMM leaves them unwritten for the T of tecm_attention_reads_q0).
 * qkv: one layer's (B,T,N,3*D) buffer exactly as tecm_attention_fwd reads it (time-major rows (b*T + p)*N + n, columns
 * [q | k | v], head h at columns h*64..); fp32, or bf16 with TECM_ATT_QKV_BF16 in `flags`.  Only q and k are read.
 * D / heads must be 64 and 1 <= T <= 1024.  T <= 32: 16 lanes per (sequence, head), the keys register-resident; 33 <= T:
 * a wave per (sequence, head), q_i in registers, the keys split over the lanes, the row's scores parked in LDS.
 *   raw export    probs (B, Ns, heads, T, T) floats; entries j > i are written as exact +0.  nodes (Ns) int32 on the device
 *                 names the nodes exported (NULL: all N in order, Ns = N); an id outside [0, N) leaves its slot all zero.
 *   accumulation  for layer slot `layer` of `num_layers` and the group g of every window b (group (B) int32 on the device,
 *                 NULL: group 0), every quantity formed in float64 from the fp32 p that is (or would be) exported, the
 *                 logarithm included, 0 ln 0 = 0:
 *                   node_stats (G, Ly, 4, N, heads): sums over the group's windows of, per sequence (b, n) and head,
 *                       [entropy (1/T) sum_i -sum_j p_ij ln p_ij, look-back (1/T) sum_i sum_j p_ij (i - j), sink (1/T) sum_i p_i0,
 *                        self (1/T) sum_i p_ii]
 *                   lag_stats (G, Ly, heads, T):  L_d = sum over sequences of sum_{i>=d} p_{i,i-d}
 *                   matrix_stats (G, Ly, heads, T, T) or NULL: sum of p_ij over sequences; T <= 32 only
 *                   counts (G) int64: windows added, advanced only with TECM_TATT_COUNT in `flags` (one layer of an update
 *                       counts, not every layer)
 *                 An id outside [0, num_groups) skips the window in every sum and sets TECM_BAD_GROUP in *err_flag, never
 *                 clamped.  No floating-point atomics: the sums over the nodes of a window go through per-block partial sums
 *                 whose tree is fixed by (N, T) alone, and every cell has ONE owning thread that adds the windows of the call in
 *                 ascending b with plain loads and stores -- the same calls in the same order give the same bits, whatever the
 *                 workspace size.
 * Either part may be left out (probs NULL / node_stats NULL), not both.  With node_stats: lag_stats, counts, err_flag and
 * num_groups, num_layers > 0 are required.
 * ws: the accumulation walks chunks of whole windows through it (4 doubles per (sequence, head), and per block of 16 (T <= 32)
 * or 4 (T > 32) nodes and head T (+ T*T with matrix_stats) doubles); 16-byte aligned.  ws_floats = floats it holds, 0 =
 * tecm_temporal_attention_ws_floats(a), which is at most 64 MiB unless one window needs more; any size that holds one window
 * is accepted (smaller: more chunks, same bits).  The export alone uses no workspace (ws may be NULL). */
#define TECM_TATT_COUNT 8                 /* flags: this call advances counts (next to TECM_ATT_QKV_BF16) */
typedef struct TecmTemporalAttn {
  const void* qkv;                        /* (B,T,N,3*D) fp32 or bf16 */
  float* probs;                           /* (B, Ns, heads, T, T) or NULL */
  const int32_t* nodes;                   /* (Ns) or NULL = all N */
  double* node_stats;                     /* (G, Ly, 4, N, heads) or NULL = no accumulation */
  double* lag_stats;                      /* (G, Ly, heads, T) */
  double* matrix_stats;                   /* (G, Ly, heads, T, T) or NULL */
  int64_t* counts;                        /* (G) */
  const int32_t* group;                   /* (B) or NULL */
  int32_t* err_flag;                      /* the device error word (TecmSpatial::err_flag) */
  float* ws; int64_t ws_floats;           /* 16-byte aligned; contents undefined after */
  int32_t B, T, N, heads, D;
  int32_t Ns;                             /* entries of `nodes`; ignored (N) when nodes is NULL */
  int32_t num_groups, num_layers, layer;  /* G, Ly, the layer slot this call adds to */
  int32_t flags;                          /* TECM_ATT_QKV_BF16 | TECM_TATT_COUNT */
} TecmTemporalAttn;
/* Floats of workspace the call asks for by default (4 when only the export is asked for, which needs none), or 0 when `a` is
 * not served.  Pure host function. */
int64_t tecm_temporal_attention_ws_floats(const TecmTemporalAttn* a);
int tecm_temporal_attention(const TecmTemporalAttn* a, void* stream);

/* ------------------------------------------------------------------ reductions / small ops
 * out[s][c] (+)= sum over rows r = o*outer_stride + j (o < outer, j < inner) + seg s offset
 * of in[r*ld + c]; row(s,o,j) = (o*nseg + s)*inner + j when nseg > 1 (wpe / bias gradients). */
int tecm_colsum(const float* in, int64_t ld, int64_t outer, int64_t inner, int32_t nseg, int32_t C,
                float* out, int64_t ldo, int32_t accumulate, float scale, const TecmDrop* in_drop,
                float* workspace /* >= 1024*nseg*C floats */, void* stream);
/* ... and, from the same pass, the (masked) input as a bf16 matrix twin[row][ld_twin] (C % 4 == 0, C <= 1024, 16-byte friendly
 * rows): a gradient whose column sums are a bias gradient (fp32 values) and which two bf16 contractions read next (the
 * rounded values) -- backward of nn.Linear / Conv1d(k=1), train.py:85. */
int tecm_colsum_twin(const float* in, int64_t ld, int64_t outer, int64_t inner, int32_t nseg, int32_t C,
                     float* out, int64_t ldo, int32_t accumulate, float scale, const TecmDrop* in_drop,
                     float* workspace, void* twin_bf16, int64_t ld_twin, void* stream);

/* nbuf matrices in[i] of the same (rows, C) shape and leading dimension ld, out[i] (C floats) = their column sums: per
 * matrix the result of tecm_colsum(in[i], ld, rows, 1, 1, C, out[i], C, 0, 1, NULL, ...) bit for bit (same blocks, same order
 * of every sum), from one pair of launches for all of them when C > 1024 or rows are not 16-byte friendly (the LayerNorm
 * backwards' (num_blocks, 2*D) partials, D = 768), else matrix by matrix.  in / out: HOST arrays of device pointers. */
int tecm_colsum_batch(const float* const* in, float* const* out, int32_t nbuf, int64_t ld, int64_t rows, int32_t C,
                      float* workspace /* >= max(1024, 256*nbuf) * C floats */, void* stream);
/* The route tecm_colsum (nbuf == 0) or tecm_colsum_batch (nbuf > 0 matrices of `outer` rows; inner = nseg = 1) takes for these
 * arguments, from the plan function the launchers route by: "v4 rb=1024 chunk=17 waves=16" -- first stage (scalar: a lane per
 * column; v4: a thread per row slot and column quad; batch: the scalar stage over a pointer table), partial rows per
 * segment, input rows per partial row, waves per 64 columns of the second stage.  A batch answers "batch rb=.. chunk=..
 * waves=.. launches=N" for its own pair(s) of launches (32 matrices a pair) and "each v4 ..." where every matrix goes through
 * tecm_colsum one by one.  "" where the launcher refuses.  in_misalign_bytes: distance of the input from a 16-byte boundary
 * (batch: of its best aligned matrix, which decides for all); the workspace is taken to be 16-byte aligned.  The environment
 * switch TECM_COLSUM_MINROWS is included.  Pure host function; the string lives until this thread's next call. */
const char* tecm_colsum_path(int64_t ld, int64_t outer, int64_t inner, int32_t nseg, int32_t C, int32_t in_misalign_bytes,
                             int32_t nbuf);

/* nn.HuberLoss(delta) mean (train.py:372) fused with its gradient: pred/target/dpred are (n) floats
 * addressed through pred_index: element e of pred = pred[e], target likewise (both contiguous in the
 * SAME logical order).  loss_out[0] = mean huber; dpred = dloss/dpred * grad_scale. */
int tecm_huber_fwd_bwd(const float* pred, const float* target, float* dpred, float* loss_out,
                       int64_t n, float delta, float grad_scale, float* workspace /* >= 1024 */,
                       void* stream);

/* Conv1d weight (Cout, Cin, k) -> GEMM operands.  fwd_pack: [Cout][k*Cin] with kk = tap*Cin + ci;
 * bwd_pack: [k*Cout][Cin] with row = tap'*Cout + co holding W[co][ci][k-1-tap'] (dX correlation). */
int tecm_conv_weight_pack(const float* w, float* fwd_pack, float* bwd_pack, int32_t Cout, int32_t Cin,
                          int32_t k, void* stream);
/* inverse of fwd_pack for the weight gradient: dW[co][ci][tap] = dpack[co][tap*Cin+ci]. */
int tecm_conv_weight_unpack(const float* dpack, float* dw, int32_t Cout, int32_t Cin, int32_t k,
                            void* stream);

/* Multi_Scale_Conv_Block (reference src/model/modules.py:43-60), bf16 mode (train.py:68): the input gradient of the three
 * parallel Conv1d(k = 3, 5, 7, padding (k-1)/2) in ONE launch that reads dy once (csrc/conv_seq.hip):
 *   dinp[b,t,n,ci] = sum_j sum_tau sum_co dy[b, t - tau + (k_j-1)/2, n, j*Cout + co] * w_j[co, ci, tau]
 * dy: bf16 (B, Lc, N, 3*Cout) time-major -- the GroupNorm+GELU backward's output; dinp: fp32 (B, Lc, N, ld_in), columns
 * >= Cin are written as zeros; wpack: the three weights (Cout, Cin, k_j) fp32 rounded to bf16 in MFMA fragment order by
 * tecm_conv_dx_pack, 15*Cout * 32*ceil(ld_in/32) bf16 values.  Cout % 64 == 0, ld_in % 4 == 0, ld_in <= 64,
 * Lc % 8 == 0; 16-byte aligned pointers. */
typedef struct TecmConvDx {
  const void* dy;
  const void* wpack;
  float* dinp;
  int32_t B, Lc, N, Cout, ld_in, _pad;
} TecmConvDx;
int tecm_conv_dx_pack(const float* w3, const float* w5, const float* w7, void* wpack, int32_t Cout, int32_t Cin,
                      int32_t ld_in, void* stream);
int tecm_conv_dx_bf16(const TecmConvDx* p, void* stream);
/* Forward of the same three Conv1d in ONE launch, bf16 mode: y (B, Lc, N, 3*Cout) fp32 = bias + conv(inp), inp bf16
 * (B, Lc, N, ld_in) with the real channels first (columns >= Cin are ignored: their weights are packed as zeros); bias =
 * b3 | b5 | b7 (3*Cout floats); wpack from tecm_conv_fwd_pack: sum_j ceil(k_j*ld_in/16) * Cout/32 * 512 bf16 values.
 * Cout % 32 == 0, Cout <= 128, ld_in % 8 == 0, Lc % 8 == 0. */
typedef struct TecmConvFwd {
  const void* inp;
  const void* wpack;
  const float* bias;
  float* y;                    /* fp32; y_bf16 != 0 (tecm_conv_fwd_bf16 only): a bf16 (B, Lc, N, 3*Cout) tensor -- what a bf16
                                  Conv1d returns under autocast (train.py:68), read by the TECM_GN_Y_BF16 norm kernels */
  int32_t B, Lc, N, Cout, ld_in, y_bf16;
  float* stats;                /* optional (tecm_conv_fwd_bf16 with y_bf16, Lc <= 48): (B*N, 3, 2) = mean, rstd of GroupNorm(1, Cout)
                                  (modules.py:28) per sequence and branch, from the ROUNDED y the kernel holds in registers -- the
                                  norm forward then is elementwise (TECM_GN_STATS_GIVEN).  NULL: not computed */
  float eps;                   /* GroupNorm eps (1e-5) */
  int32_t _pad;
} TecmConvFwd;
int tecm_conv_fwd_pack(const float* w3, const float* w5, const float* w7, void* wpack, int32_t Cout, int32_t Cin,
                       int32_t ld_in, void* stream);
int tecm_conv_fwd_bf16(const TecmConvFwd* p, void* stream);
/* ... and in exact fp32 (BASELINE configs[1], also the eval path): inp fp32, v_mfma_f32_32x32x2_f32; wpack from
 * tecm_conv_fwd_pack_f32: sum_j (k_j*ld_in/8) * Cout/32 * 256 floats. */
int tecm_conv_fwd_pack_f32(const float* w3, const float* w5, const float* w7, float* wpack, int32_t Cout, int32_t Cin,
                           int32_t ld_in, void* stream);
int tecm_conv_fwd_f32(const TecmConvFwd* p, void* stream);
/* The same in exact fp32 (BASELINE configs[1]): dy fp32, v_mfma_f32_32x32x2_f32; wpack from tecm_conv_dx_pack_f32
 * (15*Cout * 32*ceil(ld_in/32) floats). */
int tecm_conv_dx_pack_f32(const float* w3, const float* w5, const float* w7, float* wpack, int32_t Cout, int32_t Cin,
                          int32_t ld_in, void* stream);
int tecm_conv_dx_f32(const TecmConvDx* p, void* stream);
/* 1 when tecm_conv_fwd_{bf16,f32} / tecm_conv_dx_{bf16,f32} serve the shape -- divisibility AND the LDS bytes of one
 * sequence tile (64 KiB forward, 160 KiB d-input) -- else 0.  Pure host arithmetic, nothing is launched.  Callers route
 * the shapes these kernels refuse to the window-view GEMMs (tecm_gemm_*) instead of failing with TECM_E_LDS. */
int tecm_conv_fwd_supported(int32_t Lc, int32_t Cout, int32_t ld_in, int32_t f32);
int tecm_conv_dx_supported(int32_t Lc, int32_t Cout, int32_t ld_in, int32_t f32);
/* Time steps per sequence tile (TC) the launcher of that shape will use -- a sequence is walked in chunks of TC steps, the last
 * one shorter where TC does not divide Lc -- from the same plan code the launchers call; 0 where the predicate above says no.
 * Pure host arithmetic.  (tecm_conv_dw_* walks fixed chunks of 24 steps.) */
int tecm_conv_fwd_tile_steps(int32_t Lc, int32_t Cout, int32_t ld_in, int32_t f32);
int tecm_conv_dx_tile_steps(int32_t Lc, int32_t Cout, int32_t ld_in, int32_t f32);
/* 1 when one forward tile holds a whole sequence of Lc steps -- the condition for TecmConvFwd::stats -- else 0.  Pure host
 * function. */
int tecm_conv_fwd_stats_supported(int32_t Lc);

/* Weight gradient of the same three Conv1d in ONE launch pair, bf16 mode (replaces the three split-K window GEMMs
 * dY^T . window(inp) behind nn.Conv1d's autograd, modules.py:27,36):
 *   dw_j[co, ci, tau] = sum_{b,t,n} dy[b, t, n, j*Cout + co] * inp[b, t + tau - (k_j-1)/2, n, ci]     (zero outside [0, Lc))
 * inp bf16 (B, Lc, N, ld_in), dy bf16 (B, Lc, N, 3*Cout), dw3 / dw5 / dw7 fp32 (Cout, Cin, 3 / 5 / 7) -- only the Cin
 * real channels are written.  A persistent kernel of num_blocks thread blocks (one per CU is the intended use) keeps
 * all 15 taps' accumulators in registers and leaves one slab per block in `workspace`
 * (tecm_conv_dw_workspace(Cout, ld_in, num_blocks) floats); a second kernel adds the slabs in a fixed order.  Where a tile is
 * shared by two blocks (ld_in 64, Cout 128: each takes half the output channels) num_blocks = 1 launches the two, as the
 * workspace query sizes for.
 * (ld_in, Cout) in {24, 64} x {64, 128}; Lc % 4 == 0; 16-byte aligned tensors. */
typedef struct TecmConvDw {
  const void* inp;
  const void* dy;
  float* workspace;
  float* dw3;
  float* dw5;
  float* dw7;
  int32_t B, Lc, N, Cout, Cin, ld_in, num_blocks, _pad;
} TecmConvDw;
/* The same loss over a logical (B, H, N) index space with one stride triple (elements) per tensor: the model's
 * prediction is the permuted view (B, L_out, N, 1) of (B, N, L_out) storage (tec_mollm.py:122-123) and the target has its
 * own layout (train.py:76-78) -- no contiguous copies.  dpred is written with the PREDICTION's strides. */
int tecm_huber_fwd_bwd_strided(const float* pred, const int64_t* pred_strides /* 3 */, const float* target,
                               const int64_t* target_strides /* 3 */, float* dpred, float* loss_out, int32_t B, int32_t H,
                               int32_t N, float delta, float grad_scale, float* workspace /* >= 1024 */, void* stream);

int64_t tecm_conv_dw_workspace(int32_t Cout, int32_t ld_in, int32_t num_blocks);
/* 1 when tecm_conv_dw_{bf16,f32} serve the shape (the table the launcher itself refuses from), else 0.  Pure host function. */
int tecm_conv_dw_supported(int32_t Lc, int32_t Cout, int32_t ld_in);
int tecm_conv_dw_bf16(const TecmConvDw* p, void* stream);
/* The same in exact fp32 (BASELINE configs[1]): inp and dy fp32, v_mfma_f32_32x32x2_f32. */
int tecm_conv_dw_f32(const TecmConvDw* p, void* stream);

/* dst (bf16) [r][c] = round-to-nearest-even(src [r][c]) for a (rows, cols) block; cols % 4 == 0.  The cast torch.autocast
 * inserts in front of a Linear / Conv1D input (reference train.py:68), done once for a tensor a bf16 GEMM will read (here:
 * the 32 LoRA columns z = drop(LN1(h)) A^T, reference modules.py:177-186). */
int tecm_cast_bf16(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int32_t cols, void* stream);

/* bf16 forms of a trainable fp32 weight W [rows][cols] in one launch: same_bf16 = W rounded ([rows][ld_same]) and / or
 * transposed_bf16 = W^T rounded ([cols][ld_tr]) -- the values a bf16 contraction rounds W to in its loader, as tensors the
 * LDS-DMA GEMM can take as its [row][k] operand in the forward (nn.Linear / Conv1d(k=1): y = x W^T) and in the
 * input-gradient contraction (dx = dy W).  Either pointer may be NULL. */
int tecm_weight_bf16(const float* src, int64_t ld_src, void* same_bf16, int64_t ld_same, void* transposed_bf16, int64_t ld_tr,
                     int32_t rows, int32_t cols, void* stream);

/* dst[r][c] = src[r][c] * keep(seed, r*drop.ld + c) / (1 - p): the counter-based dropout mask every kernel of this
 * library recomputes (F.dropout of tec_mollm.py:115, GPT-2's embd dropout), materialised once where the masked
 * tensor is consumed several times.  cols, ld_src, ld_dst multiples of 4; 16-byte aligned. */
/* dst_bf16 != 0: dst is a bf16 tensor -- the cast autocast applies to the dropped value in front of a bf16 Linear
 * (train.py:68), done once where the masked tensor is only ever read by bf16 contractions. */
/* dst2_bf16 != NULL (dst fp32): the same masked values a second time as a bf16 tensor [r][ld_dst2] -- a gradient whose
 * column sums want the fp32 values and whose two bf16 contractions (dW, dX of the patch projection) read the rounded ones. */
int tecm_dropout_apply(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, int32_t dst_bf16, void* dst2_bf16,
                       int64_t ld_dst2, int64_t rows, int32_t cols, const TecmDrop* drop, void* stream);

/* dst[r*ldd + c] = scale * src[c*lds + r]  (r < rows, c < cols): builds the K-extended c_attn weight
 * [W ; (alpha/r) * B^T] (modules.py:177-183) and other small transposes. */
int tecm_transpose_scale(const float* src, int64_t lds, float* dst, int64_t ldd, int32_t rows,
                         int32_t cols, float scale, void* stream);

/* LoRA fold (peft Linear on c_attn, reference modules.py:177-186): writes scale * lora_B (n_out, r) into the r trainable
 * rows of the K-extended backward operand w_kn = [ W ; scale B^T ] ([k_off + r][n_out], leading dimension ld_kn) and / or
 * the r trainable columns of the forward operand w_nk = [ W^T | scale B ] ([n_out][k_off + r], ld_nk); either may be
 * NULL; *_bf16 != 0: that operand is bf16.  The frozen part of both operands is the caller's (filled once). */
int tecm_lora_fold(const float* lora_B, int32_t n_out, int32_t r, float scale, void* w_kn, int64_t ld_kn, int32_t kn_bf16,
                   void* w_nk, int64_t ld_nk, int32_t nk_bf16, int32_t k_off, void* stream);

/* dst = srcs[0] | srcs[1] | ... (count <= 12 fp32 vectors of lens[i] elements, host arrays of device pointers): the
 * per-branch bias / gamma / beta of a Multi_Scale_Conv_Block (modules.py:27-29) as the 3*Cout vectors the fused kernels
 * read, in one launch. */
int tecm_pack_vectors(const float* const* srcs, const int32_t* lens, int32_t count, float* dst, void* stream);

/* ------------------------------------------------------------------ the shell around the step
 * (2) optimizer step of train.py:92-109 + :358-366 on FLAT buffers: global-norm clip + AdamW in two
 * launches, no host sync.  Semantics of torch.nn.utils.clip_grad_norm_(max_norm) followed by
 * torch.optim.AdamW(betas, eps, weight_decay).step() (decoupled decay, bias-corrected):
 *   g      = grad * grad_scale                          (grad_scale folds the data-parallel 1/world mean)
 *   norm   = ||g||_2 over all n values ; coef = min(1, max_norm / (norm + 1e-6))   (max_norm <= 0: coef = 1)
 *   g     *= coef ; p *= 1 - lr*wd ; m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g
 *   p     -= (lr / (1-b1^step)) * m / (sqrt(v)/sqrt(1-b2^step) + eps)
 * A NaN norm gives a NaN coef (torch's clamp(max=1) keeps it): every parameter becomes NaN, as after the reference's step.
 * 1 - beta and the bias corrections are formed in double from the decimal of at most six digits that rounds to the fp32
 * beta handed over (0.999f -> 0.001, not 1.0f - 0.999f = 0.00099998713), as torch forms them from its Python floats.
 * total_norm_out[0] = norm (device scalar, optional).  zero_grad != 0 clears grad in the same pass
 * (optimizer.zero_grad(), train.py:105).  partials: >= TECM_NORM_BLOCKS doubles of workspace. */
#define TECM_NORM_BLOCKS 512
typedef struct {
  int64_t n;
  float* param; float* grad; float* exp_avg; float* exp_avg_sq;
  double* partials;
  float* total_norm_out;
  float lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale;
  int32_t step;        /* 1-based count of this update (bias correction) */
  int32_t zero_grad;
  int32_t _pad;
} TecmAdamW;
int tecm_adamw_clip_step(const TecmAdamW* a, void* stream);
/* The parameter-divergence check that rides in the step's ONE gradient all-reduce (DDP's implicit invariant, train.py:353-354:
 * every rank holds the same parameters).  tecm_checksum_tail: f64 sum of `param[0..n)` (fixed order: identical bits on ranks
 * with identical parameters), split into two floats, written into slots 2*rank, 2*rank+1 of `tail` (2*world floats: the tail
 * of the flat gradient buffer), every other slot zeroed; `ws` >= 256 doubles of scratch.  After the SUM all-reduce
 * tecm_checksum_verify ORs `bit` into the device error word when any rank's pair differs from rank 0's.  Three launches for
 * what were eleven torch-dispatched ones (tecmollm/train.py). */
int tecm_checksum_tail(const float* param, int64_t n, float* tail, int32_t world, int32_t rank, double* ws, void* stream);
int tecm_checksum_verify(const float* tail, int32_t world, int32_t* err_word, int32_t bit, void* stream);
/* *word += inc on the stream (one thread).  The step's dropout word (TecmDrop::seed_dev): recorded as the first node of a
 * captured training step, it gives every replay its own masks -- what the reference gets from torch's generator advancing
 * under F.dropout (modules.py:307, modeling_gpt2.py attn/resid/embd dropout, train.py:68-93). */
int tecm_seed_advance(uint64_t* word, uint64_t inc, void* stream);

/* (3) evaluation metrics on device (src/evaluation/metrics.py:10-89, :119-183): per prediction horizon h
 * accumulate, over all (sample, node) pairs of one batch, the sufficient statistics of
 * evaluate_metrics(): after the non-finite guard on scaled predictions (:139-145, -> 0), the
 * StandardScaler inverse transform t = y*scale + mean (:36-37, rounded to f32 twice as sklearn does
 * on f32 input), nan_to_num(nan 0, +inf 100, -inf 0) (:40-46) and the clip of predictions to
 * [clip_lo, clip_hi] = [0, 200] TECU (:50-51).  pred/target are addressed as
 * base[s*stride_s + h*stride_h + i*stride_i] (element strides), so the model's permuted output view
 * (tec_mollm.py:123) is read in place.  stats: (H, 8) doubles, ACCUMULATED across calls:
 *   [count, sum t, sum p, sum t^2, sum p^2, sum t*p, sum |t-p|, sum (t-p)^2]. */
#define TECM_METRIC_STATS 8
typedef struct {
  const float* pred; int64_t p_stride_s, p_stride_h, p_stride_i;
  const float* target; int64_t t_stride_s, t_stride_h, t_stride_i;
  int64_t S; int32_t H; int32_t _pad; int64_t I;      /* samples, horizons, values per (sample, horizon) */
  double mean, scale;                                   /* scaler.mean_[0], scaler.scale_[0]; (0,1) = already unscaled */
  float clip_lo, clip_hi; int32_t clip;                /* clip != 0: clamp predictions */
  int32_t _pad2;
  double* stats;
} TecmMetrics;
int tecm_metrics_accumulate(const TecmMetrics* m, void* stream);

/* (3b) the same eight statistics per cell (g, h, i) -- group of the sample, horizon, node -- instead of per horizon:
 * evaluate_metrics (src/evaluation/metrics.py:10-89) applied per cell, for error maps and for scores stratified by storm
 * level or time of day.  The first fields are TecmMetrics' with the same meaning and the same value pipeline (non-finite
 * scaled prediction -> 0, inverse transform with two f32 roundings, nan_to_num, optional clip of the prediction).
 *   group  (S) int32 on the device: the group of every sample; NULL = every sample is in group 0.  A sample whose id is
 *          outside [0, G) is skipped and sets TECM_BAD_GROUP in *err_flag (the device error word of TecmSpatial::err_flag:
 *          never NULL, sticky, read back by tecmollm/devcheck.py); it is never clamped into a valid group.
 *   stats  (G, H, 8, I) doubles, ((g*H + h)*8 + k)*I + i, ACCUMULATED across calls; node-contiguous, so that lanes owning
 *          neighbouring nodes read and write neighbouring doubles.
 * Every cell has ONE owning thread, which adds the cell's samples of this call in ascending s in registers and then adds
 * the eight sums to `stats` once: no atomics, so the same calls in the same order give the same bits.  Cells of a group
 * that does not occur in `group` are neither read nor written.
 * Lanes run along the nodes.  An operand with stride_i == 1 (the dataset target, a baseline -- stride_h may be 0) is read
 * in place; an operand with stride_h == 1 and stride_i == H (the model's permuted output view: 64 nodes x H horizons are
 * 64*H contiguous floats) goes through a padded LDS tile when 1 < H <= TECM_MAP_LDS_MAX_H; every other stride
 * combination, and larger H, is read in place with whatever coalescing its strides give.  All addressing is 64-bit.
 * G and ceil(H / 4) must be <= 65535 (grid dimensions). */
#define TECM_BAD_GROUP 16
#define TECM_MAP_LDS_MAX_H 32
typedef struct {
  const float* pred; int64_t p_stride_s, p_stride_h, p_stride_i;
  const float* target; int64_t t_stride_s, t_stride_h, t_stride_i;
  int64_t S; int32_t H; int32_t G; int64_t I;          /* samples, horizons, groups, nodes */
  double mean, scale;
  float clip_lo, clip_hi; int32_t clip;
  int32_t _pad2;
  double* stats;
  const int32_t* group;
  int32_t* err_flag;
} TecmMetricsMap;
int tecm_metrics_map(const TecmMetricsMap* m, void* stream);

/* (3c) probabilistic scores of a K-member ensemble per cell (g, h, i): every member and the target go through the value
 * pipeline of (3) / (3b) (non-finite scaled member -> 0, inverse transform with two f32 roundings, nan_to_num, optional clip
 * of the members only), which leaves float32 x_1..x_K and y; everything after that is float64.  With x_(1) <= ... <= x_(K)
 * the sorted members, every sum over members taken in ascending sorted order, and m = trim, per (sample, horizon, node):
 *   mu    = (sum x_(j)) / K                      var = (sum (x_(j) - mu)^2) / (K - 1)
 *   A     = (sum |x_(j) - y|) / K                D   = sum (2j - K - 1) * x_(j)     (= sum of |x_a - x_b| over unordered pairs)
 *   width = x_(K-m) - x_(1+m)                    r   = #{x_k < y} + floor(#{x_k == y} / 2), in [0, K]   (mid-rank: deterministic;
 *                                                      ties only occur where the clip or a copy makes values equal)
 * so that the ensemble CRPS is A - D / K^2 and the fair CRPS A - D / (K (K - 1)).  ACCUMULATED across samples and calls:
 *   stats  (G, H, 9, I) doubles, ((g*H + h)*9 + n)*I + i:  [count, sum y, sum mu, sum (mu-y)^2, sum |mu-y|, sum var, sum A,
 *          sum D, sum width]
 *   hist   (G, H, K+1, I) uint32, ((g*H + h)*(K+1) + r)*I + i: how often the rank was r
 * both node-contiguous.  One owning thread per cell adds the cell's samples in ascending s in registers and then adds to
 * stats / hist once: no atomics, the same calls give the same bits; cells of a group that does not occur in `group` are
 * neither read nor written; an id outside [0, G) skips the sample everywhere (the per-sample outputs included) and sets
 * TECM_BAD_GROUP in *err_flag, never clamped.
 * members are addressed as base[k*m_stride_k + s*m_stride_s + h*m_stride_h + i*m_stride_i], the target as in (3b), both
 * read in place (element strides, 64-bit); lanes run along the nodes, so m_stride_i == 1 is the coalesced layout.
 * Optional per-sample outputs (NULL skips one), float32 at out[s*o_stride_s + h*o_stride_h + i*o_stride_i]:
 *   out_mean = mu, out_std = sqrt(var), out_lo = x_(1+m), out_hi = x_(K-m)  (physical units), and
 *   out_mean_raw = the float64 mean over k ascending of the RAW members (non-finite -> 0): the ensemble-mean forecast in
 *   scaled units, the form (3) and (3b) take.
 * Limits: 2 <= K <= TECM_ENS_MAX_K, 0 <= 2*trim < K - 1, scale != 0, G and H <= 65535. */
#define TECM_ENS_STATS 9
#define TECM_ENS_MAX_K 64
typedef struct {
  const float* members; int64_t m_stride_k, m_stride_s, m_stride_h, m_stride_i;
  const float* target; int64_t t_stride_s, t_stride_h, t_stride_i;
  int64_t S; int32_t H; int32_t G; int64_t I;          /* samples, horizons, groups, nodes */
  int32_t K; int32_t trim;                             /* members, m */
  double mean, scale;
  float clip_lo, clip_hi; int32_t clip;
  int32_t _pad2;
  double* stats;
  uint32_t* hist;
  const int32_t* group;
  int32_t* err_flag;
  float* out_mean; float* out_std; float* out_lo; float* out_hi; float* out_mean_raw;
  int64_t o_stride_s, o_stride_h, o_stride_i;
} TecmEnsemble;
int tecm_ensemble_stats(const TecmEnsemble* e, void* stream);

/* (3g) split-conformal prediction intervals: nonconformity scores of a calibration split into a score store (a), the exact
 * k-th smallest score of every (group, cell) of that store (b), and the intervals those quantiles give, scored on a split or
 * emitted for a forecast (c).  Prediction and truth go through the value pipeline of (3) / (3b) (non-finite scaled prediction
 * -> 0, inverse transform with two f32 roundings, nan_to_num, optional clip of the prediction only), which leaves float32 p
 * and y; with w = max(sigma, sigma_min) (sigma: an optional per-sample scale in PHYSICAL units, e.g. an ensemble's std; a NaN
 * sigma counts as sigma_min) the score is, in float32 (csrc/conformal_score.h, ONE function for (a) and (c)),
 *   TECM_CONF_ABS:     r = |y - p|          TECM_CONF_SIGNED:  r = y - p          with sigma:  r = r / w  (one IEEE division).
 * Operands are addressed as base[s*stride_s + h*stride_h + i*stride_i] (element strides, 64-bit) and read in place; lanes run
 * along the nodes.
 *
 * (a) tecm_conformal_scores: scores[(row0 + s)*ld + h*I + i] = r(s, h, i), float32, ld >= H*I; rows outside
 *     [row0, row0 + S) and columns at or beyond H*I are not touched. */
#define TECM_CONF_ABS 0
#define TECM_CONF_SIGNED 1
#define TECM_INTERVAL_STATS 6
#define TECM_SELECT_MAX_Q 8
typedef struct {
  const float* pred; int64_t p_stride_s, p_stride_h, p_stride_i;
  const float* target; int64_t t_stride_s, t_stride_h, t_stride_i;
  const float* sigma; int64_t g_stride_s, g_stride_h, g_stride_i;     /* NULL: no scale (w = 1) */
  int64_t S; int32_t H; int32_t mode; int64_t I;       /* samples, horizons, TECM_CONF_*, nodes */
  double mean, scale;
  float clip_lo, clip_hi; int32_t clip;
  float sigma_min;                                      /* > 0 when sigma is given */
  float* scores; int64_t ld; int64_t row0;
} TecmConformalScores;
int tecm_conformal_scores(const TecmConformalScores* c, void* stream);

/* (b) tecm_column_select: out[(q*G + g)*C + c] = the ranks[g*Q + q]-th smallest (1-based) of { x[s*ld + c] : group[s] == g },
 *     for a row-major float32 store x (S, C) with leading dimension ld >= C.  A rank <= 0 gives -inf, a rank above the number
 *     of rows of the group (an empty group included) +inf; otherwise the output is the value of an actual element of exactly
 *     that rank in the numeric order with -0 and +0 adjacent and every NaN (of either sign) after +inf -- numpy's sort order.
 *     A NaN that is selected comes back as the quiet NaN 0x7fffffff.
 *   group  (S) int32 or NULL (every row in group 0); a row whose id is outside [0, G) belongs to no group and sets
 *          TECM_BAD_GROUP in *err_flag, never clamped.
 *   ranks  (G, Q) int32 on the device.
 *     Exact and bit-reproducible: a four-pass most-significant-digit radix select on 8-bit digits of the monotone key (all
 *     bits of a negative flipped, the sign bit of a non-negative set, NaN -> 0xffffffff) with integer counts only.  One block
 *     of sixteen waves serves 64 neighbouring columns of one (group, rank): lanes run along the columns, so a row is one
 *     coalesced 256-B read; the waves share the rows and count into one [256][64] uint32 histogram in LDS with LDS integer
 *     adds (lane-contiguous: a wave's update has no bank conflict); after each pass every wave walks the bins of its lane's
 *     column to the digit holding the rank.  The group id of a row is wave-uniform, so rows of other groups are not loaded.
 *     Limits: 0 < S < 2^31, 1 <= Q <= TECM_SELECT_MAX_Q, 1 <= G <= 65535, ceil(C / 64) * G * Q < 2^31 blocks. */
typedef struct {
  const float* x; int64_t ld;
  int64_t S; int64_t C;
  const int32_t* group; const int32_t* ranks;
  int32_t G; int32_t Q;
  float* out;
  int32_t* err_flag;
} TecmColumnSelect;
int tecm_column_select(const TecmColumnSelect* c, void* stream);

/* (c) tecm_interval_stats: the intervals of the quantiles q_lo, q_hi (Gq, H, I) float32 contiguous -- q_lo NULL with
 *     TECM_CONF_ABS, where q_lo = -q_hi; a sample of group g uses the quantiles of group g when Gq == G and those of group 0
 *     when Gq == 1 -- per (sample, horizon, node), with r and w as above:
 *       covered = (r <= q_hi) for ABS, (q_lo <= r <= q_hi) for SIGNED; a miss is `below` when y lies under the interval
 *                 (ABS: y < p; SIGNED: r < q_lo) and `above` otherwise
 *       lo = (float)(p + q_lo*w), hi = (float)(p + q_hi*w), evaluated in float64 from the float32 operands and rounded once,
 *                 then both clamped to [clip_lo, clip_hi] when the clip is on
 *       width = hi - lo,   Winkler score = width + (2/alpha) max(lo - y, 0) + (2/alpha) max(y - hi, 0), both in float64
 *     ACCUMULATED across samples and calls into stats (G, H, 6, I) doubles, ((g*H + h)*6 + n)*I + i:
 *       [count, covered, below, above, sum width, sum Winkler]
 *     with the layout, ownership and order of (3b): one owning thread per cell adds the cell's samples in ascending s in
 *     registers and then adds to `stats` once, no atomics; cells of a group that does not occur are neither read nor written;
 *     an id outside [0, G) skips the sample everywhere (the per-sample outputs included) and sets TECM_BAD_GROUP.
 *     Optional per-sample outputs (NULL skips one), float32 at out[s*o_stride_s + h*o_stride_h + i*o_stride_i]: out_lo, out_hi
 *     and out_mid = p.  With target == NULL only these are written (stats may be NULL, alpha is not used): the forecast path.
 *     Limits: G and ceil(H / 4) <= 65535, scale != 0, 0 < alpha < 1 with a target. */
typedef struct {
  const float* pred; int64_t p_stride_s, p_stride_h, p_stride_i;
  const float* target; int64_t t_stride_s, t_stride_h, t_stride_i;
  const float* sigma; int64_t g_stride_s, g_stride_h, g_stride_i;
  int64_t S; int32_t H; int32_t mode; int64_t I;
  double mean, scale;
  float clip_lo, clip_hi; int32_t clip;
  float sigma_min;
  const float* q_lo; const float* q_hi;
  int32_t Gq; int32_t G;
  double alpha;
  double* stats;
  const int32_t* group;
  int32_t* err_flag;
  float* out_lo; float* out_hi; float* out_mid;
  int64_t o_stride_s, o_stride_h, o_stride_i;
} TecmIntervalStats;
int tecm_interval_stats(const TecmIntervalStats* c, void* stream);

/* (3h) significance of the comparison: the eight statistics of (3) kept per WINDOW (a), and paired circular block-bootstrap
 * sums over such a table (b).  Float64 additions in a fixed, documented order, no atomics on any sum: the same call gives the
 * same bits, and tests/significance_ref.py restates both addition by addition.
 *
 * (a) tecm_metrics_window: operands, strides and value pipeline of (3) / (3b).  For every sample s and horizon h the eight
 *     statistics summed over all I nodes are WRITTEN (not accumulated) to
 *       table[(row*H + h)*8 + k],   row = rows[s] (int64, on the device), or row0 + s when rows is NULL,
 *     a table of table_rows x H x 8 doubles.  Rows that no sample names are not touched; two samples naming one row leave
 *     either.  A row outside [0, table_rows) writes nothing and sets TECM_BAD_ROW in *err_flag (never NULL, sticky).
 *     Order of the sum of one (s, h): lane l = i mod 64 of a wave adds its nodes i = l, l + 64, l + 128, ... in ascending
 *     order into a partial starting at +0.0; the 64 partials are then halved five times and once more: x[l] += x[l ^ o] for
 *     o = 32, 16, 8, 4, 2, 1 (a lane without a node holds +0.0).
 *     An operand with stride_i == 1 (stride_h may be 0) is read in place; one with stride_h == 1 and stride_i == H goes
 *     through a padded LDS tile when 1 < H <= TECM_MAP_LDS_MAX_H, as in (3b); everything else is read in place.
 *     Limits: S < 2^31, ceil(H / 4) <= 65535, scale != 0. */
#define TECM_BAD_ROW 32
#define TECM_BAD_START 64
typedef struct {
  const float* pred; int64_t p_stride_s, p_stride_h, p_stride_i;
  const float* target; int64_t t_stride_s, t_stride_h, t_stride_i;
  int64_t S; int32_t H; int32_t _pad; int64_t I;      /* samples, horizons, nodes */
  double mean, scale;
  float clip_lo, clip_hi; int32_t clip;
  int32_t _pad2;
  double* table; int64_t table_rows;
  const int64_t* rows; int64_t row0;
  int32_t* err_flag;
} TecmMetricsWindow;
int tecm_metrics_window(const TecmMetricsWindow* m, void* stream);

/* (b) tecm_block_bootstrap: table (M, S, W) doubles at table[m*stride_m + s*stride_s + w] (rows W-contiguous, stride_s >= W),
 *     starts (R, K) int32 with K == ceil(S / L), L = block length >= 1, group (S) int32 in [0, G) or NULL (group 0):
 *       out[((r*M + m)*G + g)*W + w] = sum over the positions t = 0 .. S-1, in ascending t, of table[m, row(r, t), w] for
 *       those t with group[row(r, t)] == g,   row(r, t) = (starts[r*K + t / L] + t mod L) mod S
 *     -- the circular block bootstrap, the last block truncated so that exactly S windows are read; ONE running float64 sum
 *     per output value starting at +0.0, so a sequential restatement matches bit for bit.  Every m is resampled with the
 *     same starts (paired).  A group that does not occur yields zeros; every output value is written.  A start outside
 *     [0, S) skips its block's windows and sets TECM_BAD_START, a group id outside [0, G) skips the window and sets
 *     TECM_BAD_GROUP, both in *err_flag.
 *     Limits: 0 < S < 2^31, 0 < R < 2^31, 1 <= G <= 65535, M * G * ceil(W / 64) <= 65535 (one grid dimension): any W and
 *     G <= 16 up to M = 585 at W = 400. */
typedef struct {
  const double* table; int64_t stride_m, stride_s;
  int64_t M, S, W;
  const int32_t* group; int32_t G; int32_t _pad;
  const int32_t* starts; int64_t R, K, L;
  double* out;
  int32_t* err_flag;
} TecmBlockBootstrap;
int tecm_block_bootstrap(const TecmBlockBootstrap* b, void* stream);

/* (3j) event verification: did the forecast announce the event?  Integer counts only, so every order of additions gives the
 * same bits and the tests compare with no tolerance.
 *
 * Value pipeline: the forecast (or every member) and the truth go through the value pipeline of (3) / (3b) (non-finite scaled
 * prediction -> 0, inverse transform with two f32 roundings, nan_to_num, optional clip of the prediction only), which leaves
 * float32 p (or x_1..x_K) and y in TECU.
 * Threshold: t = thr[q*th_stride_q + slot*th_stride_k + i*th_stride_i], float32 on the device, in TECU.  Any stride may be 0:
 * an absolute threshold is one float with all strides 0, a climatology-relative one a (Q, 12, N) table.  slot = slot[s*H + h],
 * an int32 (S, H) tensor on the device; NULL means slot 0 with num_slots = 1.  A slot id outside [0, num_slots) skips that
 * (sample, horizon) in every cell and sets TECM_BAD_SLOT in *err_flag (never NULL, sticky); it is never clamped.
 * Event of threshold q: v > t when dir[q] > 0, v < t when dir[q] < 0, compared in float32 and strictly: a value equal to the
 * threshold is no event, and neither is anything against a NaN threshold.  dir is a host array in the descriptor, no entry 0;
 * 1 <= Q <= TECM_EVENT_MAX_Q.
 * Groups as in (3b): an id outside [0, G) skips the sample and sets TECM_BAD_GROUP; cells of a group that does not occur in
 * the call are neither read nor written.
 *
 * (a) tecm_event_hist: K members addressed as in (3c) (base[k*m_stride_k + s*m_stride_s + h*m_stride_h + i*m_stride_i], read
 *     in place, 1 <= K <= TECM_ENS_MAX_K; K = 1 with any m_stride_k is a deterministic forecast: the model's permuted view and
 *     a stride-0 baseline view are read where they lie), the target as in (3b).  ACCUMULATED across samples and calls:
 *       hist (G, Q, H, K+1, 2, I) uint32, ((((g*Q + q)*H + h)*(K+1) + j)*2 + e)*I + i, node-contiguous:
 *         e = 0: the number of samples in which exactly j members forecast the event
 *         e = 1: how many of those samples had the event in the truth
 *     For K = 1 this IS the contingency table: o_1 hits, n_1 - o_1 false alarms, o_0 misses, n_0 - o_0 correct negatives.
 *     One wave per (tile of 64 nodes, horizon, group): lanes run along the nodes, a thread owns every count of its cell
 *     (g, ., h, ., ., i), loads its operands once per (sample, horizon, node) and compares them with all Q thresholds.  When
 *     the (K+1)*2*Q words of a node are at most TECM_EVENT_LDS_WORDS the wave counts in a column of LDS per lane and adds to
 *     `hist` once at the end; otherwise the thread reads, increments and writes the cells it owns in `hist`.  No atomics.
 *     Limits: G and H <= 65535, scale != 0, all addressing 64-bit. */
#define TECM_BAD_SLOT 128
#define TECM_EVENT_MAX_Q 8
#define TECM_EVENT_LDS_WORDS 256
typedef struct {
  const float* members; int64_t m_stride_k, m_stride_s, m_stride_h, m_stride_i;
  const float* target; int64_t t_stride_s, t_stride_h, t_stride_i;
  int64_t S; int32_t H; int32_t G; int64_t I;          /* samples, horizons, groups, nodes */
  int32_t K; int32_t Q;                                /* members, thresholds */
  double mean, scale;
  float clip_lo, clip_hi; int32_t clip;
  int32_t num_slots;
  const float* thr; int64_t th_stride_q, th_stride_k, th_stride_i;
  const int32_t* slot;
  int32_t dir[TECM_EVENT_MAX_Q];
  uint32_t* hist;
  const int32_t* group;
  int32_t* err_flag;
} TecmEventHist;
int tecm_event_hist(const TecmEventHist* e, void* stream);

/* (b) tecm_event_fss: the sums of the fractions skill score (Roberts & Lean 2008) of a deterministic forecast on a
 *     rows x cols grid, node i = r*cols + c, I == rows*cols.  Per (sample, horizon, threshold) Bf, Bo are the binary event
 *     fields of forecast and truth and cf(x), co(x) their box sums over the n x n window centred on x, cells outside the grid
 *     counting as no event (zero padding).  For W odd widths n_w (host array, 1 <= W <= TECM_EVENT_MAX_W, 1 <= n <= 127),
 *     ACCUMULATED across samples and calls:
 *       sums (G, Q, H, W, 3) uint64, (((g*Q + q)*H + h)*W + w)*3 + n:  [sum_x (cf - co)^2, sum_x cf^2, sum_x co^2]
 *     The common 1 / n^4 cancels: FSS = 1 - sums[0] / (sums[1] + sums[2]) is formed on the host.
 *     One block per (sample, horizon): the event bits of all Q thresholds of both fields are staged in LDS once (a byte per
 *     node and field), then per threshold two summed-area tables are built there and the widths walked; a block adds its
 *     3 W integer sums per threshold to `sums` with 64-bit integer atomic adds (integers: order-free, the same bits).
 *     The largest grid follows from the LDS map (768 B of reduction space, 8 (rows+1) (cols+1) B of tables, 2 I B of bits, in
 *     64 KiB) and is answered by tecm_event_fss_supported(rows, cols) (pure host, 1 = served); 41 x 71 takes 30.1 KiB.
 *     Limits: S and H <= 65535, scale != 0. */
#define TECM_EVENT_MAX_W 8
typedef struct {
  const float* pred; int64_t p_stride_s, p_stride_h, p_stride_i;
  const float* target; int64_t t_stride_s, t_stride_h, t_stride_i;
  int64_t S; int32_t H; int32_t G; int64_t I;          /* samples, horizons, groups, nodes */
  int32_t rows, cols;
  int32_t Q; int32_t W;                                /* thresholds, widths */
  double mean, scale;
  float clip_lo, clip_hi; int32_t clip;
  int32_t num_slots;
  const float* thr; int64_t th_stride_q, th_stride_k, th_stride_i;
  const int32_t* slot;
  int32_t dir[TECM_EVENT_MAX_Q];
  int32_t widths[TECM_EVENT_MAX_W];
  uint64_t* sums;
  const int32_t* group;
  int32_t* err_flag;
} TecmEventFss;
int tecm_event_fss(const TecmEventFss* e, void* stream);
int tecm_event_fss_supported(int32_t rows, int32_t cols);

/* (4) sliding-window batch assembly from device-resident series (SlidingWindowSamplerDataset.__getitem__
 * src/data/dataset.py:65-99 + the harness reshapes train.py:62-65, :76): for sample b with window
 * start a = starts[b] (already multiplied by the dataset stride):
 *   x_out[b, t, :, :]   = X[a + t, :, :]                       t < L_in     (B, L_in, N*C) contiguous
 *   tf_out[b, t, :]     = TF[a + t, :]                                       (B, L_in, F_t)
 *   y_out[b, h, i]      = Y[a + L_in - 1, i, h]                h < L_out    (B, L_out, N): the target
 *                         already in the (B, L_out, N, 1) order of train.py:76
 * X (T, N*C), TF (T, F_t), Y (T, N, L_out), starts (B) int64 on the device.  Out-of-range windows are
 * rejected on the host only when starts_host_check is given (same values, host memory); the kernel
 * clamps nothing. */
typedef struct {
  const float* X; const float* TF; const float* Y; const int64_t* starts;
  const int64_t* starts_host_check;
  int64_t T; int64_t row; /* N*C floats per time step */
  int32_t N, L_in, L_out, F_t, B, _pad;
  float* x_out; float* tf_out; float* y_out;
} TecmWindowBatch;
int tecm_window_batch(const TecmWindowBatch* w, void* stream);

/* (5) per-window baseline forecasts straight from the device-resident series (the second half of the reference's test.py):
 * for window b with start a = starts[b] (already multiplied by the dataset stride), node n < N and horizon h < L_out, with
 * x(t) = X[t*N*C + n*C + channel]:
 *   TECM_BASELINE_MEAN      out[b,h,n] = (((x(a) + x(a+1)) + ...) + x(a+L_in-1)) / (float)L_in -- the historical average of
 *                           get_baseline_predictions (test.py:57-62).  fp32 adds in ascending time order, then ONE IEEE fp32
 *                           division: the bits numpy's np.mean(x_window[:, :, :, 0:1], axis=0) returns for an fp32 window.
 *   TECM_BASELINE_LAST      out[b,h,n] = x(a + L_in - 1)                                    (persistence; not in the reference)
 *   TECM_BASELINE_PERIODIC  out[b,h,n] = x(a + L_in - period + (h mod period))              (the same slot one period ago: with
 *                           period = 12 two-hourly steps, yesterday; not in the reference).  Needs L_in >= period > 0.
 * All three read channel `channel` of the feature-scaled X as it is, as the reference's baseline does, although the targets
 * they are scored against carry the target scaler.
 * out is addressed as out[b*o_stride_b + h*o_stride_h + n*o_stride_n] (element strides).  o_stride_h may be 0 for MEAN and
 * LAST (every horizon holds the same value: it is then written once -- the (B, L_out, N, 1) forecast as a stride-0 view);
 * PERIODIC with L_out > 1 needs o_stride_h != 0.  X (T, N*C) fp32, starts (B) int64 on the device; windows are range-checked
 * on the host when starts_host_check is given (same values, host memory) and a window outside [0, T - L_in] that reaches
 * the kernel is written as NaN, never read. */
enum { TECM_BASELINE_MEAN = 0, TECM_BASELINE_LAST = 1, TECM_BASELINE_PERIODIC = 2 };
typedef struct {
  const float* X; const int64_t* starts;
  const int64_t* starts_host_check;
  int64_t T;
  int32_t N, C, channel, L_in, L_out, B, mode, period;
  float* out; int64_t o_stride_b, o_stride_h, o_stride_n;
} TecmWindowBaseline;
int tecm_window_baseline(const TecmWindowBaseline* w, void* stream);

/* (6) HistoricalAverage.fit (src/models/baselines.py:13-33): the mean of a series per node and time-of-day slot,
 *   means[n*n_slots + s] = sum over { t < T : slot[t] == s } of x[t*stride_t + n*stride_n]  /  counts[s]
 * x fp32 addressed by element strides ((T, N) data, or one channel of (T, N*C) in place), slot (T) int32 on the device
 * (values outside [0, n_slots) belong to no slot), means (N, n_slots) and counts (n_slots) doubles.  Sums are fp64 in
 * ascending time order inside four fixed quarters of T that are then added as (q0 + q1) + (q2 + q3); no atomics, so two
 * launches return identical bits.  An empty slot yields NaN (numpy's mean of an empty selection). */
typedef struct {
  const float* x; int64_t stride_t, stride_n;
  const int32_t* slot;
  int64_t T; int32_t N, n_slots;
  double* means; double* counts;
} TecmSlotMean;
int tecm_slot_mean(const TecmSlotMean* m, void* stream);

/* (7) SarimaBaseline (src/models/baselines.py:47-72) on the device: a seasonal ARMA on the differenced series in subset
 * (additive) form, estimated per node by the two-stage Hannan-Rissanen regression.  NOT statsmodels' exact-likelihood
 * multiplicative SARIMAX: the lags of the expanded product polynomials each carry a free coefficient, there is no constant,
 * and nothing iterates.  Everything below is fp64; the series is fp32.
 *   lags      ar_lags[n_ar], ma_lags[n_ma] ascending and positive, K = n_ar + n_ma in [1, TECM_SAR_MAX_K], the largest lag
 *             Lmax <= TECM_SAR_MAX_LAG, Lmax <= m <= TECM_SAR_MAX_LONG_AR, d and D in {0, 1}, s >= 1 when D = 1, and the
 *             differencing offset o = d + s*D <= TECM_SAR_MAX_OFFSET.
 *   w_u       = (y_t - y_{t-1}) - (y_{t-s} - y_{t-s-1}) with t = u + o (d = D = 1; y_t - y_{t-1} for d alone, y_t - y_{t-s}
 *             for D alone, y_t for neither), u < n = T - o.
 *   stage 1   autocov[k] = (1/n) sum_{u=k}^{n-1} w_u w_{u-k}, k <= m; Levinson-Durbin gives the long AR phi^(m);
 *             e_u = w_u - sum_{i<=m} phi_i w_{u-i}, u >= m.
 *   stage 2   rows u = m + Lmax .. n-1, z_u = [w_{u-a}]_{a in ar_lags} ++ [e_{u-b}]_{b in ma_lags}; gram = [G | r] with
 *             G = sum z z^T, r = sum z w_u; Cholesky solve -> coef = (phi_A, theta_M); sigma2 = residual mean square
 *             (wss - 2 coef.r + coef.G.coef) / rows with wss = sum w_u^2 over the rows.
 *   status    TECM_SAR_NONFINITE: a NaN / inf in the node's series (coef and sigma2 NaN).  TECM_SAR_DEGENERATE: autocov[0] <= 0,
 *             a Levinson variance <= 0, a Cholesky pivot <= 1e-12 G_kk, or n < m + Lmax + 2K (coef 0, sigma2 = autocov[0]: the
 *             forecast is then the differencing rule alone).  TECM_SAR_MA_DROPPED: solved with use_ma[node] == 0.
 * tecm_sar_fit: x addressed by element strides ((T, N) data, or one channel of (T, N*C) in place).  The time axis is cut
 * into fixed chunks of TECM_SAR_CHUNK steps of u; a block (64 nodes, lanes along nodes) sums one chunk in ascending time
 * after rebuilding its rings of w and e from the steps before it, and the chunks are joined in ascending order: no atomics,
 * two calls return identical bits.  ws: tecm_sar_fit_ws_bytes() bytes, 8-byte aligned.
 * tecm_sar_solve: solves again from gram / wss / autocov (as tecm_sar_fit left them); use_ma (N) int8 or NULL; a node with
 * use_ma == 0 solves the leading n_ar x n_ar block with theta = 0.  Keeps the stage-1 bits of status. */
enum { TECM_SAR_MAX_K = 12, TECM_SAR_MAX_LAG = 32, TECM_SAR_MAX_LONG_AR = 64, TECM_SAR_MAX_OFFSET = 64, TECM_SAR_CHUNK = 1024 };
enum { TECM_SAR_DEGENERATE = 1, TECM_SAR_NONFINITE = 2, TECM_SAR_MA_DROPPED = 4 };
typedef struct {
  const float* x; int64_t stride_t, stride_n;
  int64_t T;
  int32_t N, d, D, s, m, n_ar, n_ma, _pad;
  int32_t ar_lags[12], ma_lags[12];
  double* autocov;        /* (N, m+1) */
  double* gram;           /* (N, K, K+1) = [G | r] */
  double* wss;            /* (N) sum of w_u^2 over the stage-2 rows */
  double* coef;           /* (N, K) */
  double* sigma2;         /* (N) */
  int32_t* status;        /* (N) */
  const int8_t* use_ma;   /* (N) or NULL; read by tecm_sar_solve only */
  double* ws;             /* tecm_sar_fit only */
} TecmSarFit;
int64_t tecm_sar_fit_ws_bytes(const TecmSarFit* f);     /* pure host arithmetic; -1 on a bad descriptor */
int tecm_sar_fit(const TecmSarFit* f, void* stream);
int tecm_sar_solve(const TecmSarFit* f, void* stream);

/* SarimaBaseline's forecast (src/models/baselines.py:64-72, there only from the end of the training series) for every window
 * of a split in one launch: TecmWindowBaseline's fields (mode and period unused; o_stride_h != 0 when L_out > 1) plus the
 * coefficients.  For window b, node n, in fp64: w over the window; e_u = 0 for u < Lmax, then e_u = w_u - sum phi_a w_{u-a}
 * - sum theta_b e_{u-b}; for the future w^_u = sum phi_a w_{u-a} + sum theta_b e_{u-b} with future e = 0 and future w = w^;
 * y^ = w^ integrated back through the differencing rule, earlier forecasts standing in where a lag reaches them; rounded to
 * fp32 at the store.  Needs L_in >= o + Lmax + 1.  coef (N, K) doubles as tecm_sar_fit writes it.  A window outside
 * [0, T - L_in] that reaches the kernel is written as NaN, never read. */
typedef struct {
  TecmWindowBaseline w;
  const double* coef;
  int32_t d, D, s, n_ar, n_ma, _pad;
  int32_t ar_lags[12], ma_lags[12];
} TecmSarForecast;
int tecm_sar_forecast(const TecmSarForecast* f, void* stream);

/* (8) the raw-data stage on the device (scripts/preprocess.py over src/features/feature_engineering.py).
 *
 * (a) tecm_moments: what StandardScaler.fit computes (feature_engineering.py:161-170 for X, preprocess.py:56-60 for Y)
 *     over a strided 2-D view src[r*ld + c], r < rows, c < cols, float32 (src_f64 = 0) or float64 (src_f64 = 1):
 *       pool = 1  one statistic over every column (TEC: the reference reshapes to one feature)
 *       pool = 0  one statistic per column (cols of them)
 *       taps = 0  every row has weight 1
 *       taps = H  row r has the integer weight  w_r = max(0, min(H-1, r-1) - max(0, r - rows + H) + 1):  the number of
 *                 times construct_target_tensor_Y (feature_engineering.py:55-67) writes row r into Y (rows - H, ..., H), so
 *                 that the fit equals StandardScaler().fit(Y.reshape(-1, 1)) without the H-fold tensor.  Needs taps < rows.
 *     Per statistic, on the device:  count (int64) = sum of w over the non-NaN entries (NaN entries are skipped, as
 *     sklearn's nansum does), mean (fp64) = sum w x / count, var (fp64) = sum w (x - mean)^2 / count (population); a
 *     statistic with count 0 gets NaN mean and var.  Two passes, the mean stays on the device in between; no host
 *     synchronisation, no atomics, a fixed combination order: the same bits on every call.
 *     Accuracy contract: every thread adds its entries through a cascade of seven accumulators that carry every 64 adds
 *     (at most 63 dependent additions per level, 16 on the last: rows*cols < 2^40), a block joins its 256 threads by a
 *     tree of 8, and one block joins the at most TECM_MOMENTS_MAX_BLOCKS partials of a statistic by 8 sequential adds
 *     and a tree of 8: fewer than 512 dependent fp64 additions into any output, under the 4096 the bound of
 *     4096 * 2^-53 = 4.6e-13 (relative to the mean of |x|, and of (x - mean)^2) allows.
 *     ws: tecm_moments_ws_bytes() bytes, 8-byte aligned (pure host arithmetic; -1 on a bad descriptor). */
#define TECM_MOMENTS_MAX_BLOCKS 2048
typedef struct {
  const void* src; int64_t rows, cols, ld;
  int32_t src_f64, pool, taps, _pad;
  int64_t* count; double* mean; double* var;
  void* ws;
} TecmMoments;
int64_t tecm_moments_ws_bytes(const TecmMoments* m);
int tecm_moments(const TecmMoments* m, void* stream);

/* (b) tecm_features_build: construct_feature_tensor_X, construct_target_tensor_Y (feature_engineering.py:38-67),
 *     standardize_features (:179-192) and the Y scaling of preprocess.py:75-83 for one split in one call, from
 *     tec (rows, N) float32 / float64 (tec_f64) and idx (rows, Ci) float32 / float64 (idx_f64) on the device; mean and
 *     scale are HOST arrays of 1 + Ci doubles (the fitted feature scaler), ymean / yscale the target scaler.  Outputs, all
 *     float32, contiguous, each optional (NULL skips it):
 *       X  (x_rows, N, 1 + Ci)   X[t, n, 0] = f32((f64(tec[t, n]) - mean[0]) / scale[0])
 *                                X[t, n, 1 + k] = f32((f64(idx[t, k]) - mean[1 + k]) / scale[1 + k])       x_rows <= rows
 *       Ys (rows, N)             Ys[t, n] = f32((f64(tec[t, n]) - ymean) / yscale)
 *       Y  (rows - H, N, H)      Y[t, n, h] = the Ys value of tec[t + 1 + h, n]: the reference's materialised layout
 *     Exactly one fp64 subtraction, one correctly rounded fp64 division and one round-to-nearest-even conversion per value
 *     (no reciprocal, no contraction): the bits StandardScaler.transform followed by .float() gives.  NaN passes through.
 *     Threads run along consecutive output floats; float4 stores on 16-byte aligned quads of the output with scalar stores
 *     for the quads a row boundary cuts, scalar everywhere for a pointer that is not 16-byte aligned.
 *     Limits: 0 <= Ci <= TECM_FEATURES_MAX_CI, every scale non-zero, 0 < H < rows with Y. */
#define TECM_FEATURES_MAX_CI 15
typedef struct {
  const void* tec; const void* idx;
  int64_t rows, x_rows; int32_t N, Ci, H, tec_f64, idx_f64, _pad;
  const double* mean; const double* scale;
  double ymean, yscale;
  float* X; float* Ys; float* Y;
} TecmFeaturesBuild;
int tecm_features_build(const TecmFeaturesBuild* f, void* stream);

/* (c) tecm_window_batch_series: tecm_window_batch (4) with the target taken from the target-scaled series Ys (Ty, N)
 *     instead of the reference's materialised Y (src/data/dataset.py:88-93 reads Y[a + L_in - 1], which
 *     feature_engineering.py:63-65 filled with rows a + L_in .. a + L_in + L_out - 1 of the series):
 *       x_out, tf_out   as in (4)
 *       y_out[b, h, :]  = Ys[starts[b] + L_in + h, :]           h < L_out      (B, L_out, N)
 *     so one resident series serves every L_out and a batch's target is L_out contiguous row copies.  With
 *     starts_host_check the host rejects a window outside [0, T - L_in] and, with y_out, one whose last target row
 *     starts[b] + L_in + L_out - 1 lies outside the Ty rows of Ys. */
typedef struct {
  const float* X; const float* TF; const float* Ys; const int64_t* starts;
  const int64_t* starts_host_check;
  int64_t T; int64_t Ty; int64_t row; /* N*C floats per time step of X */
  int32_t N, L_in, L_out, F_t, B, _pad;
  float* x_out; float* tf_out; float* y_out;
} TecmWindowBatchSeries;
int tecm_window_batch_series(const TecmWindowBatchSeries* w, void* stream);

/* (9) LinearBaseline (not in the reference, whose PRD section 3 calls its baseline zoo extensible): a direct linear map from
 * the input window to the H targets, fitted per node by ridge regression -- the "Linear" family of the LLM-forecaster
 * ablations.  The first baseline here that is FITTED against the target-scaled series; (5) reads the feature-scaled channel
 * as it is.  Everything below is fp64; X and ys are fp32.
 *   predictors  z = [1, X[a + L_in - lag[p], n, chan[p]] for p = 1 .. P-1] for the window that starts at row a: P counts the
 *               intercept, entry 0 of chan / lag is ignored, 1 <= lag[p] <= min(L_in, TECM_LIN_MAX_LAG) (lag 1 is the last
 *               input step), 0 <= chan[p] < C with at most TECM_LIN_MAX_CHANNELS distinct channels.
 *   targets     y_h = ys[(a + L_in + h) * ys_stride_t + n * ys_stride_n], h < H (element strides, Ty rows).
 *   windows     a = first + i * step, i < count: an arithmetic progression, first >= 0, step >= 1, count >= 1, the last
 *               window's inputs inside the T rows of X and its targets inside the Ty rows of ys.
 *   model       W_n = argmin sum_a |y - z^T W|^2 + alpha sum_{p >= 1} |W_p|^2 (the intercept is not penalised): sklearn's
 *               Ridge(alpha, fit_intercept=True) in exact arithmetic.  Pooled: one W from the sum of the nodes' normal
 *               equations.
 * tecm_lin_gram writes gram (N, P, P+H) = [G | R], G = sum_a z z^T, R = sum_a z y^T.  Every entry is ONE running fp64 sum
 * over the windows in ascending order; the factors are fp32 values, so every product is exact in fp64 and a fused
 * multiply-add equals multiply-then-add.  Hence no atomics, no split of the time axis and no workspace; G is bitwise
 * symmetric (the full P x (P+H) rectangle is computed), two launches return identical bits, and a sequential loop over
 * the windows on the host reproduces them bit for bit.  With pooled != 0 it also writes gram_pooled (P, P+H): the nodes'
 * arrays added in ascending node order, one chain per entry.
 * A block owns a tile of nodes for the whole series and walks it in chunks of windows staged in LDS (at most 64 KiB);
 * tecm_lin_gram_supported is pure host arithmetic: 1 when the descriptor's shape is served (pointers are not looked at), else
 * 0 with the reason in tecm_last_error; tile_nodes / chunk_windows (either may be NULL) receive the geometry the launch uses. */
enum { TECM_LIN_MAX_P = 64, TECM_LIN_MAX_H = 32, TECM_LIN_MAX_LAG = 512, TECM_LIN_MAX_CHANNELS = 8 };
enum { TECM_LIN_DEGENERATE = 1, TECM_LIN_NONFINITE = 2 };
typedef struct {
  const float* X; int64_t T;                    /* (T, N*C) */
  const float* ys; int64_t ys_stride_t, ys_stride_n, Ty;
  int32_t N, C, P, H, L_in, pooled;
  int32_t chan[TECM_LIN_MAX_P], lag[TECM_LIN_MAX_P];
  int64_t first, step, count;
  double* gram;           /* (N, P, P+H) */
  double* gram_pooled;    /* (P, P+H) when pooled */
} TecmLinGram;
int tecm_lin_gram_supported(const TecmLinGram* g, int32_t* tile_nodes, int32_t* chunk_windows);
int tecm_lin_gram(const TecmLinGram* g, void* stream);

/* tecm_lin_solve: for each of the N systems gram (N, P, P+H) (N = 1 for a pooled fit), the Cholesky solve of
 * (G + alpha diag(0, 1, ..., 1)) W = R with H right-hand sides: coef (N, P, H) and, when coef_t is given, the same values
 * node-fastest (P, H, N), the layout tecm_lin_forecast reads.  status (N): any non-finite entry of [G | R] gives
 * TECM_LIN_NONFINITE and NaN coefficients; a pivot <= 1e-12 x its diagonal entry (of G + alpha D) gives TECM_LIN_DEGENERATE
 * and the intercept-only model coef[0, h] = R[0, h] / G[0, 0], other rows 0: the forecast is the mean training target. */
typedef struct {
  const double* gram;
  int32_t N, P, H, _pad;
  double alpha;
  double* coef; double* coef_t;
  int32_t* status;
} TecmLinSolve;
int tecm_lin_solve(const TecmLinSolve* s, void* stream);

/* tecm_lin_forecast: TecmWindowBaseline's fields (channel, mode and period unused; o_stride_h != 0 when L_out > 1; L_out is
 * the fitted H) plus the predictor pairs and the coefficients: coef is node-fastest, coef[(p*H + h)*N + n], with
 * coef_stride_n = 1, or one (P, H) array for every node with coef_stride_n = 0 (pooled).
 *   out[b, h, n] = (float)(coef[0, h] + z_1 coef[1, h] + ... + z_{P-1} coef[P-1, h]), p ascending, in fp64.
 * One launch for any number of windows; a window outside [0, T - L_in] that reaches the kernel is written as NaN, never
 * read. */
typedef struct {
  TecmWindowBaseline w;
  const double* coef; int64_t coef_stride_n;
  int32_t P, _pad;
  int32_t chan[TECM_LIN_MAX_P], lag[TECM_LIN_MAX_P];
} TecmLinForecast;
int tecm_lin_forecast(const TecmLinForecast* f, void* stream);

/* (10) AnalogBaseline (not in the reference): the analog ensemble, the non-parametric baseline of space-weather and NWP
 * post-processing.  For every (query window, node) the K stretches of the node's training record that lie nearest to the
 * query's last m input steps are found, and what followed them is the forecast: K members, and their mean.
 *   archive     A (N, Ta) fp32 NODE-MAJOR: A[n*Ta + r] is the feature-scaled channel of node n at row r.  The outcomes are
 *               read by tecm_analog_forecast from Y (N, Ty), node-major too, whose row r is the same instant as row r of A.
 *   candidates  a start row c of a segment A[c .. c+m-1]; its origin is o_c = c + m and its outcome Y[o_c + h], h < L_out.
 *               Valid: 0 <= c, c + m <= Ta, c + m + L_out <= Ty.
 *   queries     window b starts at row a = starts[b] of Xq (Tq, N*C) (time-major, as a dataset holds it); its segment is
 *               Xq[(a + L_in - m + l)*N*C + n*C + channel], l < m, and its origin o_q = a + L_in + origin_shift (the shift
 *               maps a row of Xq to the archive's row numbering; it only enters the exclusion rule).
 *   distance    d = sum_{l<m} (A[c+l] - q[l])^2 in fp32, every term rounded (difference, fused multiply-add).  A candidate
 *               whose d is NaN or +inf is never selected, so a query segment that holds a NaN selects nothing.
 *   admission   keys (key_arch (Tk) and key_q (S) int32, both or neither): only candidates with key_arch[o_c] == key_q[b];
 *               needs Tk > the last candidate's origin.  exclude > 0: only candidates with |o_c - o_q| >= exclude.
 *   selection   the K admitted candidates smallest by (d, c) -- on equal distance the earlier row -- ascending in that order:
 *               idx (S, N, K) int32, dist (S, N, K) fp32, unused places -1 / +inf, count (S, N) int32 = min(K, admitted).
 * The order (d, c) is total, so the result does not depend on the launch geometry and two calls return identical bits.
 * A block owns (one node, a tile of queries) and sweeps the node's archive in chunks staged in LDS; the distances are never
 * stored.  tecm_analog_search_supported is pure host arithmetic: 1 when the descriptor's shape is served (no pointer is
 * followed; key_arch != NULL says that keys are in use, which Tk must then cover), else 0 with the reason in tecm_last_error; chunk / query_tile / n_candidates (each may be NULL) receive the
 * candidates per staged chunk, the queries per block and the number of valid candidates.  Windows are range-checked on the
 * host when starts_host_check is given; a window outside [0, Tq - L_in] that reaches the kernel selects nothing. */
enum { TECM_ANALOG_MAX_K = 32, TECM_ANALOG_MAX_M = 512, TECM_ANALOG_MAX_H = 32 };
typedef struct {
  const float* A; int64_t Ta;                   /* (N, Ta) node-major */
  int64_t Ty;                                   /* rows of the outcome series: bounds the candidates */
  const float* Xq; int64_t Tq;                  /* (Tq, N*C) */
  const int64_t* starts; const int64_t* starts_host_check;
  int64_t origin_shift;
  int32_t N, C, channel, L_in, L_out, m, K, S;
  const int32_t* key_arch; int64_t Tk;          /* NULL: no keys */
  const int32_t* key_q;
  int32_t exclude, _pad;                        /* 0: no exclusion */
  int32_t* idx; float* dist; int32_t* count;
} TecmAnalogSearch;
int tecm_analog_search_supported(const TecmAnalogSearch* s, int32_t* chunk, int32_t* query_tile, int64_t* n_candidates);
int tecm_analog_search(const TecmAnalogSearch* s, void* stream);

/* tecm_analog_forecast: from idx / count as tecm_analog_search wrote them (B = S windows) and the outcomes Y (N, Ty):
 *   members[((k*B + b)*L_out + h)*N + n] = Y[n*Ty + idx[b,n,k] + m + h] for k < count[b,n], NaN for the others
 *                                          (K, B, L_out, N) contiguous, the layout of the ensemble statistics (3d)
 *   out[b*o_stride_b + h*o_stride_h + n*o_stride_n] = (float)(fp64 sum of the count members, k ascending, / count),
 *                                          NaN where count == 0; a NaN outcome propagates
 * Either output may be NULL.  An index whose outcome row would leave the Ty rows is not read and counts as NaN. */
typedef struct {
  const float* Y; int64_t Ty;                   /* (N, Ty) node-major */
  const int32_t* idx; const int32_t* count;
  int32_t N, K, m, L_out, B, _pad;
  float* out; int64_t o_stride_b, o_stride_h, o_stride_n;
  float* members;
} TecmAnalogForecast;
int tecm_analog_forecast(const TecmAnalogForecast* f, void* stream);

/* (3k) quantile forecasts: the pinball loss a quantile model is trained with (a), the scores a Q-level forecast is judged
 * by per cell (g, h, i) (b), and the nonconformity score of conformalized quantile regression (c).
 *
 * LAYOUT CONVENTION (the one place it is stated): levels taus = (tau_1 < ... < tau_Q), 1 <= Q <= TECM_QUANT_MAX_Q, every
 * tau in (0, 1).  A quantile model is TEC_MoLLM built with prediction_horizon = Q * L_out; output channel j = q*L_out + h
 * holds level q (0-based) of horizon h, so out.view(B, Q, L_out, N) -- strided, no copy -- is the quantile tensor and level q
 * alone a (B, L_out, N, 1) view.
 *
 * (a) tecm_pinball_fwd_bwd_strided: the mean pinball loss of pred (B, Q, H, N) against target (B, H, N), fused with its
 *     gradient.  pred is addressed as pred[b*p_stride_b + q*p_stride_q + h*p_stride_h + n*p_stride_n], target as
 *     target[b*t_stride_b + h*t_stride_h + n*t_stride_n] (element strides, 64-bit, read in place).  With M = B*H*N and
 *       u   = y - p                                   (float32)
 *       rho = (double)u * ((double)tau_q - [u < 0])   (float64)
 *     the outputs are
 *       loss_levels[q] = (float)((sum of rho over level q) / M)                  (optional, Q floats)
 *       loss_out[0]    = (float)((sum of the Q level sums, q ascending) / (Q*M))
 *       dpred          = g * ([u < 0] - tau_q),  g = grad_scale / (float)(Q*M)   (optional; float32: one division, one
 *                        subtraction and one product), written at pred's offsets: dpred has pred's layout.
 *     At u == 0 the gradient is the -tau branch ([u < 0] = 0): d rho / d p = -tau there, as for every u > 0.
 *     Order of the sums (float64, fixed, no atomics): block (x, q) of nbx = min(ceil(M / 256), TECM_PINBALL_BLOCK_CAP) x Q
 *     blocks of 256 threads walks the elements e = x*256 + t, + nbx*256, ... of level q's (b, h, n) space in ascending
 *     order per thread; the 64 partials of a wave are halved six times (v += v[l ^ o], o = 32 .. 1), the four waves added as
 *     (w0 + w1) + (w2 + w3) into workspace[q*nbx + x]; a second one-block stage adds every level's nbx partials the same
 *     way (thread t: x = t, t + 256, ...).  Element e decodes with h fastest when p_stride_n != 1 (the head's (B, N, Q*H)
 *     storage: p_stride_h == 1) and with n fastest when p_stride_n == 1, so lanes run along whichever is contiguous.
 *     workspace: Q * nbx doubles.  Limits: Q*M < 2^53; no value is filtered: a NaN operand gives a NaN loss. */
#define TECM_QUANT_MAX_Q 16
#define TECM_PINBALL_BLOCK_CAP 1024
typedef struct {
  const float* pred; int64_t p_stride_b, p_stride_q, p_stride_h, p_stride_n;
  const float* target; int64_t t_stride_b, t_stride_h, t_stride_n;
  int32_t B, Q, H, N;
  float taus[TECM_QUANT_MAX_Q];
  float grad_scale; int32_t _pad;
  float* dpred;                  /* NULL: loss only */
  float* loss_out;
  float* loss_levels;            /* NULL: not wanted */
  double* workspace;
} TecmPinball;
int tecm_pinball_fwd_bwd_strided(const TecmPinball* p, void* stream);

/* (b) tecm_quantile_stats: the Q levels, addressed as levels[q*l_stride_q + s*l_stride_s + h*l_stride_h + i*l_stride_i], and
 *     the target (as in (3b)) go through the value pipeline of (3) / (3b) (non-finite scaled value -> 0, inverse transform
 *     with two f32 roundings, nan_to_num, optional clip of the levels only), which leaves float32 x_1..x_Q and y.  Per
 *     (sample, horizon, node), with P = Q / 2 (integer division):
 *       crossing c = [there is a q with x_q > x_{q+1}]
 *       z        = x sorted ascending (the rearrangement), then z_q = z_q + adjust[((ga*H + h)*Q + q)*I + i] in float32 when
 *                  adjust (Ga, H, Q, I) is given; ga = g when Ga == G and 0 when Ga == 1
 *       rho_q    = ((double)y - (double)z_q) * ((double)tau_q - [y < z_q])
 *       hit b_q  = [y <= z_q]
 *       pair r = 1..P:  lo = z_r, hi = z_{Q+1-r};  width = (double)hi - (double)lo (negative where adjust makes it so: not
 *                  clamped),  covered = [lo <= y <= hi]
 *     (one device function, quantile_sorted in csrc/quantile.hip, gives (c) the same z and y).  ACCUMULATED across samples and
 *     calls into two node-contiguous arrays, index ((g*H + h)*(1 + Q + P) + n)*I + i:
 *       stats   doubles: [count, sum rho_1..rho_Q, sum width_1..width_P]
 *       counts  uint32:  [crossings, hits_1..hits_Q, covered_1..covered_P]
 *     with the ownership and order of (3c): one wave per (tile of 64 nodes, horizon, group), lanes along the nodes, one
 *     owning thread per cell adds its samples in ascending s in registers and adds to the arrays once: no atomics, the same
 *     calls give the same bits; cells of a group that does not occur are neither read nor written; an id outside [0, G)
 *     skips the sample everywhere and sets TECM_BAD_GROUP in *err_flag.  Q is served by the compile-time bucket 1, 2, 4, 8
 *     or 16 (padding +inf sorts behind the finite levels).  Optional per-sample output: out_z[q*o_stride_q + s*o_stride_s +
 *     h*o_stride_h + i*o_stride_i] = z_q, the (adjusted) sorted levels in physical units.  With target == NULL only out_z is
 *     written (stats and counts may be NULL): the forecast path.
 *     Limits: 1 <= Q <= TECM_QUANT_MAX_Q, G and H <= 65535, scale != 0. */
typedef struct {
  const float* levels; int64_t l_stride_q, l_stride_s, l_stride_h, l_stride_i;
  const float* target; int64_t t_stride_s, t_stride_h, t_stride_i;
  int64_t S; int32_t H; int32_t G; int64_t I;          /* samples, horizons, groups, nodes */
  int32_t Q; int32_t Ga;                               /* levels; groups of adjust (1 or G) */
  float taus[TECM_QUANT_MAX_Q];
  double mean, scale;
  float clip_lo, clip_hi; int32_t clip;
  int32_t _pad2;
  const float* adjust;           /* NULL: none */
  double* stats;
  uint32_t* counts;
  const int32_t* group;
  int32_t* err_flag;
  float* out_z; int64_t o_stride_q, o_stride_s, o_stride_h, o_stride_i;
} TecmQuantileStats;
int tecm_quantile_stats(const TecmQuantileStats* c, void* stream);

/* (c) tecm_quantile_scores: the CQR score (Romano, Patterson and Candes 2019) of the pair (lo_idx, hi_idx), 0-based indices
 *     into the SORTED levels z of (b) (no adjust), in float32:
 *       E = max(z_lo - y, y - z_hi),   scores[(row0 + s)*ld + h*I + i] = E
 *     -- the addressing of tecm_conformal_scores (3g)(a), so tecm_column_select selects from the store unchanged.  The
 *     interval [z_lo - Qhat, z_hi + Qhat] covers y exactly when E <= Qhat.
 *     Limits: 0 <= lo_idx <= hi_idx < Q, ld >= H*I, row0 >= 0, ceil(H / 4) <= 65535, scale != 0. */
typedef struct {
  const float* levels; int64_t l_stride_q, l_stride_s, l_stride_h, l_stride_i;
  const float* target; int64_t t_stride_s, t_stride_h, t_stride_i;
  int64_t S; int32_t H; int32_t Q; int64_t I;
  int32_t lo_idx, hi_idx;
  double mean, scale;
  float clip_lo, clip_hi; int32_t clip;
  int32_t _pad2;
  float* scores; int64_t ld; int64_t row0;
} TecmQuantileScores;
int tecm_quantile_scores(const TecmQuantileScores* c, void* stream);

/* (3l) forecast combination (Bates-Granger / Granger-Ramanathan): a least-squares fit, per cell (g, h, i), of the truth on
 * M forecasts of it with an intercept.  Three steps: the moments of a fitting pass (a), the per-cell solve (b) and the blend
 * of a batch of forecasts with fitted coefficients (c).  Everything works on the raw float32 values as the forecasts and the
 * dataset's target hold them -- the scaled domain, BEFORE the value pipeline of (3) -- and every product and sum is float64.
 * An operand (a member forecast, the target) is a base pointer with element strides, read in place at
 * base[s*stride_s + h*stride_h + i*stride_i] (64-bit): the model's permuted view has stride_h = 1, stride_i = H, targets and
 * Linear / SARIMA forecasts are node-contiguous, the mean / last baselines are stride_h = 0 views.
 *
 * (a) tecm_combine_moments: with z = [1, p_1 .. p_M, t] per (sample, horizon, node), a cell accumulates the upper triangle,
 *     row-major, of the (M+2) x (M+2) matrix sum z z^T -- entry (a, b), a <= b, at k = a*(M+2) - a*(a-1)/2 + (b - a), the
 *     first being the count n -- followed by one double `skipped`: K = (M+2)(M+3)/2 + 1 doubles.  A sample in which any
 *     member or the target is non-finite is left out of every moment of its cell and counted in `skipped`.
 *       stats  (G, H, K, I) doubles, ((g*H + h)*K + k)*I + i, node-contiguous as in (3b), ACCUMULATED across calls.
 *     Ownership, order and groups as in (3b): one owning thread per cell adds its samples in ascending s in registers and
 *     adds to `stats` once; no atomics, the same calls give the same bits, and sums of dyadic values are exact.  Cells of a
 *     group that does not occur are neither read nor written; an id outside [0, G) skips the sample and sets
 *     TECM_BAD_GROUP in *err_flag, never clamped.  Block shape of (3b) (lane = node, wave = horizon); an operand with
 *     stride_h == 1 and stride_i == H goes through the padded LDS tile when 1 < H <= TECM_MAP_LDS_MAX_H, every other one is
 *     read in place: the route does not change a bit of the result.  M is served by the compile-time bucket 1, 2, 4 or 8
 *     (padded members contribute nothing and are not stored).
 *     Limits: 1 <= M <= TECM_COMBINE_MAX_MEMBERS, G and ceil(H / 4) <= 65535. */
#define TECM_COMBINE_MAX_MEMBERS 8
typedef struct {
  const float* base; int64_t stride_s, stride_h, stride_i;
} TecmCombineOperand;
typedef struct {
  TecmCombineOperand member[TECM_COMBINE_MAX_MEMBERS];   /* the first M are read */
  TecmCombineOperand target;
  int64_t S; int32_t H; int32_t G; int64_t I;            /* samples, horizons, groups, nodes */
  int32_t M; int32_t _pad;
  double* stats;
  const int32_t* group;          /* (S) int32; NULL: every sample in group 0 */
  int32_t* err_flag;
} TecmCombineMoments;
int tecm_combine_moments(const TecmCombineMoments* c, void* stream);

/* (b) tecm_combine_solve: one thread per cell of `stats`, addressed as stats[g*s_stride_g + h*s_stride_h + k*s_stride_k +
 *     i*s_stride_i] (element strides; G*H*I cells).  With the moments of (a):
 *       n = count,  pbar = sum p / n,  tbar = sum t / n
 *       C_ab = sum p_a p_b - n pbar_a pbar_b,   c_a = sum p_a t - n pbar_a tbar
 *       A = C + ridge*n*I,                      b = c + ridge*n*w0
 *     A is factorised by Cholesky in member order.  Member m is DROPPED when A_mm <= 0 or its pivot A_mm - sum over kept
 *     k < m of L_mk^2 is <= TECM_COMBINE_PIVOT_TOL * A_mm: it gets weight 0 and bit m of the cell's `dropped` byte, and the
 *     kept members solve their own system.  intercept = tbar - w^T pbar.  No fused multiply-add is used, so a restatement
 *     that performs the same operations in the same order gives the same bits.
 *       weight (G, H, M, I) doubles, intercept (G, H, I) doubles, status (G, H, I) int32, dropped (G, H, I) uint8.
 *     status bits: TECM_COMBINE_EMPTY (n = 0: prior weights w0, intercept 0), TECM_COMBINE_FEW (0 < n < M + 2: prior
 *     weights, intercept tbar - w0^T pbar), TECM_COMBINE_DROPPED (at least one member dropped), TECM_COMBINE_NONFINITE (a
 *     non-finite moment: prior weights, intercept 0; tested first).  The M buckets of (a).
 *     Limits: 1 <= M <= TECM_COMBINE_MAX_MEMBERS, ridge >= 0, G*H*I < 2^31 * 256. */
#define TECM_COMBINE_EMPTY 1
#define TECM_COMBINE_FEW 2
#define TECM_COMBINE_DROPPED 4
#define TECM_COMBINE_NONFINITE 8
#define TECM_COMBINE_PIVOT_TOL 1e-10
typedef struct {
  const double* stats; int64_t s_stride_g, s_stride_h, s_stride_k, s_stride_i;
  int32_t G; int32_t H; int64_t I;                       /* cells: G * H * I */
  int32_t M; int32_t _pad;
  double ridge;
  double w0[TECM_COMBINE_MAX_MEMBERS];                   /* the prior; the first M are read */
  double* weight; double* intercept; int32_t* status; uint8_t* dropped;
} TecmCombineSolve;
int tecm_combine_solve(const TecmCombineSolve* c, void* stream);

/* (c) tecm_combine_apply: out[s*o_stride_s + h*o_stride_h + i*o_stride_i] = (float)(intercept[g, h, i] + sum over m
 *     ascending of weight[g, h, m, i] * p_m[s, h, i]), accumulated in float64 and rounded once.  The coefficients are
 *     addressed as weight[g*w_stride_g + h*w_stride_h + m*w_stride_m + i*w_stride_i] and intercept[g*b_stride_g +
 *     h*b_stride_h + i*b_stride_i] (element strides, any of which may be 0: pooled fits).  A non-finite member propagates.
 *     A sample whose id is outside [0, G) gets a NaN row and sets TECM_BAD_GROUP in *err_flag.
 *     Limits: 1 <= M <= TECM_COMBINE_MAX_MEMBERS, ceil(H / 4) <= 65535. */
typedef struct {
  TecmCombineOperand member[TECM_COMBINE_MAX_MEMBERS];
  int64_t S; int32_t H; int32_t G; int64_t I;
  int32_t M; int32_t _pad;
  const double* weight; int64_t w_stride_g, w_stride_h, w_stride_m, w_stride_i;
  const double* intercept; int64_t b_stride_g, b_stride_h, b_stride_i;
  float* out; int64_t o_stride_s, o_stride_h, o_stride_i;
  const int32_t* group;          /* (S) int32; NULL: every sample in group 0 */
  int32_t* err_flag;
} TecmCombineApply;
int tecm_combine_apply(const TecmCombineApply* c, void* stream);

/* (3m) multivariate scores of a K-member ensemble per (sample s, horizon h): the energy score and the variogram score
 * (Scheuerer & Hamill 2015).  The scores of (3c) look at one cell at a time: permuting the members independently at every
 * node leaves every one of them bit for bit the same.  These two look at the member as a MAP.
 * Members and truth go through the value pipeline of (3c), unchanged (non-finite scaled member -> 0, inverse transform with two
 * f32 roundings, nan_to_num, optional clip of the members only), which leaves float32 x_k[i], k < K, and y[i], i < I.
 *
 * Energy score -- everything after the pipeline is float64, ||.|| the Euclidean norm over the I nodes:
 *   A = (1/K) sum_k ||x_k - y||      D = sum_{k<k'} ||x_k - x_k'||      E = ||mean_k x_k - y||    (the mean: k ascending, / K)
 *   ES = A - D / K^2,  fair ES = A - D / (K (K - 1))  (NaN for K = 1), as the CRPS follows from A and D of (3c).  K = 1 is allowed:
 *   ES of a point forecast is its Euclidean error E.
 * Variogram score of order p, with f_p(d) = sqrt(d), d, d^2 for order = TECM_FIELD_ORDER_HALF / _ONE / _TWO (p = 0.5, 1, 2) --
 * for every pair i < j whose class c = pair_class[i*I + j] is < NB:
 *   v_o = f_p(|y_i - y_j|)      v_e = (sum_k f_p(|x_ki - x_kj|)) / K      e = v_o - v_e
 *   in float32 (difference, square root to 1 ulp, the sum over k ascending, one division); e, e^2 and every sum over pairs,
 *   samples or calls in float64.  Per (s, h, c): the number of pairs, sum e^2 (the score of the class), sum v_o and sum v_e
 *   (the observed and the ensemble variogram: their ratio says whether the members are too smooth or too rough at that distance).
 *   pair_class  (I, I) uint8 on the device, read only above the diagonal; a value >= NB excludes the pair.  NULL with NB = 0:
 *               the energy score only.
 * Outputs, ACCUMULATED across samples and calls:
 *   es_stats (G, H, 4) doubles [n, sum A, sum D, sum E];   vs_stats (G, H, NB, 5) doubles [n, sum pairs, sum e^2, sum v_o, sum v_e]
 * and, optional (NULL skips one), per sample and OVERWRITTEN: es_out (S, H, 3) doubles [A, D, E], vs_out (S, H, NB, 4) doubles
 * [pairs, sum e^2, sum v_o, sum v_e]; the rows of a skipped sample are not written.
 * Groups as in (3c): an id outside [0, G) skips the sample everywhere and sets TECM_BAD_GROUP in *err_flag; cells of a group
 * that does not occur are neither read nor written.  members / target are addressed as in (3c) (element strides, read in
 * place; node-contiguous is the coalesced layout).
 * No atomics on the sums: blocks write partial sums to the workspace (tile pairs of T x T nodes for the variogram, up to
 * TECM_FIELD_ENERGY_SPLITS node ranges for the norms), small kernels add them in a fixed order, and one thread per
 * (g, h[, c]) adds the samples in ascending s -- two identical calls give identical bits.
 * tecm_field_scores_plan is pure host arithmetic (no pointer is followed): 1 when the shape is served, with the node tile T,
 * the dynamic LDS bytes of the largest kernel and the workspace bytes (each pointer may be NULL), else 0 with the reason
 * in tecm_last_error.
 * Limits: 1 <= K <= TECM_ENS_MAX_K, 0 <= NB <= TECM_FIELD_MAX_CLASSES, S and H <= TECM_FIELD_MAX_GRID, ceil(I / T) <=
 * TECM_FIELD_MAX_TILES, scale != 0. */
enum { TECM_FIELD_ORDER_HALF = 0, TECM_FIELD_ORDER_ONE = 1, TECM_FIELD_ORDER_TWO = 2 };
#define TECM_FIELD_MAX_CLASSES 16
#define TECM_FIELD_THREADS 256
#define TECM_FIELD_ENERGY_SPLITS 8
#define TECM_FIELD_MAX_GRID 65535
#define TECM_FIELD_MAX_TILES 65535
#define TECM_FIELD_ES_STATS 4
#define TECM_FIELD_VS_STATS 5
typedef struct {
  const float* members; int64_t m_stride_k, m_stride_s, m_stride_h, m_stride_i;
  const float* target; int64_t t_stride_s, t_stride_h, t_stride_i;
  int64_t S; int32_t H; int32_t G; int64_t I;          /* samples, horizons, groups, nodes */
  int32_t K; int32_t NB;                               /* members, pair classes */
  double mean, scale;
  float clip_lo, clip_hi; int32_t clip;
  int32_t order;                                       /* TECM_FIELD_ORDER_* */
  const uint8_t* pair_class;
  double* es_stats; double* vs_stats;
  double* es_out; double* vs_out;
  const int32_t* group;
  int32_t* err_flag;
  void* workspace; int64_t workspace_bytes;
} TecmFieldScores;
int tecm_field_scores_plan(int64_t S, int32_t H, int64_t I, int32_t K, int32_t NB, int32_t* tile, int64_t* lds_bytes,
                           int64_t* workspace_bytes);
int tecm_field_scores(const TecmFieldScores* f, void* stream);

/* (3n) reordering of ensemble members by a dependence template (ensemble copula coupling, Schefzik et al. 2013; the Schaake
 * shuffle, Clark et al. 2004): what makes K calibrated values per cell into K maps.  It replaces the torch route -- two stable
 * argsorts, a sort and take_along_dim on a materialised (K, S, H, I) template -- by one pass that reads 2 K floats and writes K
 * floats per cell.  The scores of (3c) are unchanged by it, bit for bit; those of (3m) are what it is judged by.
 * Per cell (s, h, i), under the total order "a before b":  a < b orders numbers;  equal numbers order by member index, lower
 * first, and -0.0 equals +0.0;  a NaN comes after every number, NaNs among themselves by member index --
 *   r_k            the position of template member k in that order, in [0, K)
 *   v_(0..K-1)     the K values of the cell in that order
 *   out[k,s,h,i] = v_(r_k)
 * so the output holds exactly the cell's input values, bit patterns included (NaN payloads, the sign of a zero).  No value
 * pipeline: the operands are compared as they are.
 * values, the member template and out are addressed as base[k*stride_k + s*stride_s + h*stride_h + i*stride_i] (element strides,
 * 64-bit, read and written in place; lanes run along the nodes, so stride_i == 1 is the coalesced layout).
 * Template, one of
 *   member tensor  rows == NULL: tmpl is (K, S, H, I) with t_stride_k/s/h/i.
 *   dated rows     rows != NULL, (S, K) int32 on the device, contiguous: tmpl is a series of T rows and
 *                  template[k,s,h,i] = tmpl[(rows[s*K + k] + h)*t_stride_row + i*t_stride_i]   (t_stride_k/s/h are not used),
 *                  read in place: a (T, I) series has t_stride_row = I, t_stride_i = 1, a node-major (I, T) one t_stride_row = 1,
 *                  t_stride_i = T.  A sample with rows[s*K + k] < 0 or rows[s*K + k] + H > T for any k reads nothing of the
 *                  series: every out[., s, ., .] is NaN, every out_rank[., s, ., .] is 255, and TECM_BAD_ROW is set in
 *                  *err_flag (the sticky device error word of (3b); never NULL with rows).  Nothing is clamped.
 * out_rank (optional, NULL skips it): (K, S, H, I) uint8, contiguous, r_k.
 * Aliasing: out may be the very view values is (same pointer, same four strides): the owner of a cell reads its K values before
 * it writes them.  Every other overlap of out or out_rank with an operand (compared by the byte ranges the strides span) is
 * TECM_E_ARG, and so is a zero stride of out along an axis longer than 1.
 * One wave per (tile of 64 nodes, h, s); K is served by the compile-time bucket 2, 4, 8, 16, 32 or 64 >= K, as in (3c).
 * Limits: 2 <= K <= TECM_ENS_MAX_K, S and H <= TECM_REORDER_MAX_GRID, with rows T >= H. */
#define TECM_REORDER_MAX_GRID 65535
typedef struct {
  const float* values; int64_t v_stride_k, v_stride_s, v_stride_h, v_stride_i;
  const float* tmpl; int64_t t_stride_k, t_stride_s, t_stride_h, t_stride_i;
  const int32_t* rows; int64_t t_stride_row; int64_t T;  /* dated template only */
  float* out; int64_t o_stride_k, o_stride_s, o_stride_h, o_stride_i;
  uint8_t* out_rank;
  int64_t S; int32_t H; int32_t K; int64_t I;          /* samples, horizons, members, nodes */
  int32_t* err_flag;
} TecmMemberReorder;
int tecm_member_reorder(const TecmMemberReorder* r, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TECMOLLM_H */
