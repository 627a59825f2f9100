// Event verification on the device: tecm_event_hist and tecm_event_fss (include/tecmollm.h (3j)), the kernels under
// EventMetrics (src/evaluation/metrics.py) -- contingency tables, the Brier / reliability / ROC histogram of an ensemble and
// the sums of the fractions skill score without a host copy of the forecasts.  Everything either kernel produces is an
// integer count: every order of additions gives the same bits.
//
// event_hist_kernel: block (x, y, z) = (tile of 64 nodes, horizon h, group g), ONE wave, the shape of ensemble_stats_kernel:
// lane = node of the tile, so a thread owns every count of its cell and needs no atomics.  It walks the samples in ascending
// s, takes those whose group is g and whose slot is valid, loads the truth and the K members once (the next sample's truth
// and first eight members are already in flight while the current one is compared), runs each through the value pipeline of
// metrics_value.h and compares it with all Q thresholds; the Q member counts j_q live in statically indexed registers.  The
// count (q, j_q) is a run-time index, so the counters cannot be registers:
//   LDS = true   (K+1)*2*Q <= TECM_EVENT_LDS_WORDS = 256 words per node: a column of LDS per lane ([word][lane], so a wave's
//                update has no bank conflict and a lane touches its own column only: no barrier), added to `hist` once at the
//                end.  At most 64 KiB per block; K = 1, Q = 4 takes 4 KiB, K = 16, Q = 4 takes 34 KiB.
//   LDS = false  larger K * Q (K = 64 with Q >= 2): the thread reads, increments and writes its own cells of `hist` in global
//                memory, two per (sample, threshold).  Slower per sample, but such a histogram does not fit beside anything.
// The kernel is bound by each wave's serial walk over its samples (a load round trip per sample, hidden one deep), not by
// bytes: K + 1 floats are read per (sample, horizon, node) and nothing is written until the end.
//
// event_fss_kernel: block (x, y) = (horizon h, sample s), 256 threads.  Step 1: a thread per node loads forecast and truth
// once, runs the pipeline and packs the Q event bits of either field into one byte per node in LDS.  Step 2, per threshold:
// the two binary fields become summed-area tables P[(rows+1)][(cols+1)] of uint32 in LDS (a thread per row adds along the
// row, then a thread per column adds down the column), and for every width a thread per node takes the two clipped box sums
// from four table reads each (cells outside the grid hold no event: the window is clipped to the grid), squares in integers
// and the block reduces the three uint64 sums by wave shuffles and one LDS round; Q * W * 3 atomic 64-bit integer adds per
// block go to `sums`.  41 x 71 takes 30.1 KiB of LDS.
#include "common.h"
#include "metrics_value.h"

namespace {

constexpr int EV_TILE = 64;                  // nodes per block = lanes of the wave
constexpr int EV_HEAD = 8;                   // members of the next sample kept in flight

__device__ __forceinline__ float event_value(float v, double mean, double scale, bool pred, int clip, float lo, float hi) {
  if (pred && !isfinite(v)) v = 0.f;
  v = nan_to_num_tec(unscale_f32(v, mean, scale));
  if (pred && clip) v = fminf(fmaxf(v, lo), hi);
  return v;
}

__device__ __forceinline__ bool is_event(float v, float t, int dir) { return dir > 0 ? v > t : v < t; }

template <bool LDS>
__global__ __launch_bounds__(EV_TILE) void event_hist_kernel(TecmEventHist q) {
  extern __shared__ uint32_t cnt[];          // LDS: [(q*(K+1) + j)*2 + e][lane]
  const unsigned lane = threadIdx.x;
  const int g = blockIdx.z;
  const int64_t h = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * EV_TILE + lane;
  const bool own = i < q.I;
  const int K = q.K, Q = q.Q, K1 = q.K + 1;
  const int words = K1 * 2 * Q;
  if (LDS)
    for (int w = 0; w < words; ++w) cnt[w * EV_TILE + lane] = 0u;

  bool bad_group = false, bad_slot = false;
  const bool scan_slots = q.slot && blockIdx.x == 0 && blockIdx.z == 0;    // these blocks look at the slot of every sample
  int slot_cur = 0, slot_nxt = 0;
  // the block's next sample at or after s (block-uniform) with its slot; every id is looked at exactly once
  auto next_match = [&](int64_t s, int& slot) {
    for (; s < q.S; ++s) {
      const int id = q.group ? q.group[s] : 0;
      if ((unsigned)id >= (unsigned)q.G) bad_group = true;
      const bool take = id == g;
      if (take || scan_slots) {
        slot = q.slot ? q.slot[s * q.H + h] : 0;
        const bool ok = (unsigned)slot < (unsigned)q.num_slots;
        if (!ok) bad_slot = true;
        if (take && ok) break;
      }
    }
    return s;
  };
  auto load_head = [&](float (&x)[EV_HEAD], float& y, int64_t s) {
    const float* base = q.members + s * q.m_stride_s + h * q.m_stride_h + i * q.m_stride_i;
#pragma unroll
    for (int k = 0; k < EV_HEAD; ++k) x[k] = (own && k < K) ? base[(int64_t)k * q.m_stride_k] : 0.f;
    y = own ? q.target[s * q.t_stride_s + h * q.t_stride_h + i * q.t_stride_i] : 0.f;
  };

  float thr[TECM_EVENT_MAX_Q];
  auto load_thr = [&](int slot) {
    const float* base = q.thr + (int64_t)slot * q.th_stride_k + i * q.th_stride_i;
#pragma unroll
    for (int t = 0; t < TECM_EVENT_MAX_Q; ++t) thr[t] = (own && t < Q) ? base[(int64_t)t * q.th_stride_q] : 0.f;
  };
  if (q.th_stride_k == 0) load_thr(0);       // the thresholds do not depend on the sample

  float cur[EV_HEAD], nxt[EV_HEAD], ycur = 0.f, ynxt = 0.f;
  int64_t s = next_match(0, slot_cur);
  bool present = false;
  if (s < q.S) load_head(cur, ycur, s);
  while (s < q.S) {
    present = true;
    const int64_t s2 = next_match(s + 1, slot_nxt);
    if (s2 < q.S) load_head(nxt, ynxt, s2);
    if (own) {
      if (q.th_stride_k != 0) load_thr(slot_cur);
      int j[TECM_EVENT_MAX_Q];
#pragma unroll
      for (int t = 0; t < TECM_EVENT_MAX_Q; ++t) j[t] = 0;
#pragma unroll
      for (int k = 0; k < EV_HEAD; ++k) {
        if (k < K) {
          const float v = event_value(cur[k], q.mean, q.scale, true, q.clip, q.clip_lo, q.clip_hi);
#pragma unroll
          for (int t = 0; t < TECM_EVENT_MAX_Q; ++t) j[t] += (t < Q && is_event(v, thr[t], q.dir[t])) ? 1 : 0;
        }
      }
      const float* base = q.members + s * q.m_stride_s + h * q.m_stride_h + i * q.m_stride_i;
      for (int k0 = EV_HEAD; k0 < K; k0 += EV_HEAD) {                      // K > 8: the rest, eight loads at a time
        float x[EV_HEAD];
#pragma unroll
        for (int k = 0; k < EV_HEAD; ++k) x[k] = (k0 + k < K) ? base[(int64_t)(k0 + k) * q.m_stride_k] : 0.f;
#pragma unroll
        for (int k = 0; k < EV_HEAD; ++k) {
          if (k0 + k < K) {
            const float v = event_value(x[k], q.mean, q.scale, true, q.clip, q.clip_lo, q.clip_hi);
#pragma unroll
            for (int t = 0; t < TECM_EVENT_MAX_Q; ++t) j[t] += (t < Q && is_event(v, thr[t], q.dir[t])) ? 1 : 0;
          }
        }
      }
      const float y = event_value(ycur, q.mean, q.scale, false, 0, 0.f, 0.f);
#pragma unroll
      for (int t = 0; t < TECM_EVENT_MAX_Q; ++t) {
        if (t < Q) {
          const uint32_t o = is_event(y, thr[t], q.dir[t]) ? 1u : 0u;
          if (LDS) {
            const int w = (t * K1 + j[t]) * 2;
            cnt[w * EV_TILE + lane] += 1u;
            cnt[(w + 1) * EV_TILE + lane] += o;
          } else {
            uint32_t* cell = q.hist + (((((int64_t)g * Q + t) * q.H + h) * K1 + j[t]) * 2) * q.I + i;
            cell[0] += 1u;
            cell[q.I] += o;
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < EV_HEAD; ++k) cur[k] = nxt[k];
    ycur = ynxt;
    slot_cur = slot_nxt;
    s = s2;
  }
  if (lane == 0) {
    if (bad_group && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) atomicOr(q.err_flag, TECM_BAD_GROUP);
    if (bad_slot && scan_slots) atomicOr(q.err_flag, TECM_BAD_SLOT);
  }
  if (!LDS || !present || !own) return;
  for (int t = 0; t < Q; ++t) {
    uint32_t* cell = q.hist + ((((int64_t)g * Q + t) * q.H + h) * K1 * 2) * q.I + i;
    for (int w = 0; w < K1 * 2; ++w) {
      const uint32_t c = cnt[(t * K1 * 2 + w) * EV_TILE + lane];
      if (c) cell[(int64_t)w * q.I] += c;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- FSS
constexpr int FSS_THREADS = 256;
constexpr int FSS_RED_BYTES = TECM_EVENT_MAX_W * (FSS_THREADS / 64) * 3 * 8;    // 768
constexpr int64_t FSS_LDS_MAX = 64 * 1024;

inline int64_t fss_lds_bytes(int64_t rows, int64_t cols) {
  return FSS_RED_BYTES + 8 * (rows + 1) * (cols + 1) + ((2 * rows * cols + 7) & ~(int64_t)7);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(FSS_THREADS) void event_fss_kernel(TecmEventFss q) {
  extern __shared__ unsigned long long fss_lds[];
  const int rows = q.rows, cols = q.cols, I = rows * cols, ld = cols + 1, psize = (rows + 1) * ld;
  unsigned long long* red = fss_lds;                                       // [w][wave][3]
  uint32_t* sat = reinterpret_cast<uint32_t*>(fss_lds + FSS_RED_BYTES / 8);   // [field][rows+1][cols+1]
  uint8_t* bits = reinterpret_cast<uint8_t*>(sat + 2 * psize);             // [field][I]: bit t = event of threshold t
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t h = blockIdx.x, s = blockIdx.y;
  const int Q = q.Q, W = q.W;

  const int g = q.group ? q.group[s] : 0;
  if ((unsigned)g >= (unsigned)q.G) {        // block-uniform
    if (tid == 0 && h == 0) atomicOr(q.err_flag, TECM_BAD_GROUP);
    return;
  }
  const int slot = q.slot ? q.slot[s * q.H + h] : 0;
  if ((unsigned)slot >= (unsigned)q.num_slots) {
    if (tid == 0) atomicOr(q.err_flag, TECM_BAD_SLOT);
    return;
  }

  // step 1: the event bits of every threshold, both fields
  for (int i = tid; i < I; i += FSS_THREADS) {
    const float p = event_value(q.pred[s * q.p_stride_s + h * q.p_stride_h + (int64_t)i * q.p_stride_i], q.mean, q.scale,
                                true, q.clip, q.clip_lo, q.clip_hi);
    const float y = event_value(q.target[s * q.t_stride_s + h * q.t_stride_h + (int64_t)i * q.t_stride_i], q.mean, q.scale,
                                false, 0, 0.f, 0.f);
    const float* tb = q.thr + (int64_t)slot * q.th_stride_k + (int64_t)i * q.th_stride_i;
    unsigned bf = 0, bo = 0;
#pragma unroll
    for (int t = 0; t < TECM_EVENT_MAX_Q; ++t) {
      if (t < Q) {
        const float thr = tb[(int64_t)t * q.th_stride_q];
        bf |= (is_event(p, thr, q.dir[t]) ? 1u : 0u) << t;
        bo |= (is_event(y, thr, q.dir[t]) ? 1u : 0u) << t;
      }
    }
    bits[i] = (uint8_t)bf;
    bits[I + i] = (uint8_t)bo;
  }
  // row 0 and column 0 of both tables are zero for every threshold
  for (int e = tid; e < 2 * ld; e += FSS_THREADS) sat[(e / ld) * psize + e % ld] = 0u;
  for (int e = tid; e < 2 * (rows + 1); e += FSS_THREADS) sat[(e / (rows + 1)) * psize + (e % (rows + 1)) * ld] = 0u;
  __syncthreads();

  for (int t = 0; t < Q; ++t) {
    // step 2a: prefix sums along every row of both fields
    for (int e = tid; e < 2 * rows; e += FSS_THREADS) {
      const int f = e / rows, r = e - f * rows;
      const uint8_t* b = bits + f * I + r * cols;
      uint32_t* P = sat + f * psize + (r + 1) * ld + 1;
      uint32_t run = 0;
      for (int c = 0; c < cols; ++c) {
        run += (b[c] >> t) & 1u;
        P[c] = run;
      }
    }
    __syncthreads();
    // step 2b: and down every column
    for (int e = tid; e < 2 * cols; e += FSS_THREADS) {
      const int f = e / cols, c = e - f * cols;
      uint32_t* P = sat + f * psize + c + 1;
      uint32_t run = 0;
      for (int r = 1; r <= rows; ++r) {
        run += P[r * ld];
        P[r * ld] = run;
      }
    }
    __syncthreads();
    // step 3: the widths
#pragma unroll
    for (int w = 0; w < TECM_EVENT_MAX_W; ++w) {
      if (w < W) {
        const int half = q.widths[w] >> 1;
        unsigned long long a0 = 0, a1 = 0, a2 = 0;
        for (int i = tid; i < I; i += FSS_THREADS) {
          const int r = i / cols, c = i - r * cols;
          const int r0 = max(r - half, 0), r1 = min(r + half, rows - 1) + 1;
          const int c0 = max(c - half, 0), c1 = min(c + half, cols - 1) + 1;
          const uint32_t* Pf = sat;
          const uint32_t* Po = sat + psize;
          const uint32_t cf = Pf[r1 * ld + c1] - Pf[r0 * ld + c1] - Pf[r1 * ld + c0] + Pf[r0 * ld + c0];
          const uint32_t co = Po[r1 * ld + c1] - Po[r0 * ld + c1] - Po[r1 * ld + c0] + Po[r0 * ld + c0];
          const long long d = (long long)cf - (long long)co;
          a0 += (unsigned long long)(d * d);
          a1 += (unsigned long long)cf * cf;
          a2 += (unsigned long long)co * co;
        }
        a0 = wave_sum_u64(a0);
        a1 = wave_sum_u64(a1);
        a2 = wave_sum_u64(a2);
        if (lane == 0) {
          unsigned long long* o = red + (w * (FSS_THREADS / 64) + wave) * 3;
          o[0] = a0; o[1] = a1; o[2] = a2;
        }
      }
    }
    __syncthreads();
    if (tid < W * 3) {
      const int w = tid / 3, n = tid - w * 3;
      unsigned long long v = 0;
#pragma unroll
      for (int k = 0; k < FSS_THREADS / 64; ++k) v += red[(w * (FSS_THREADS / 64) + k) * 3 + n];
      unsigned long long* cell = reinterpret_cast<unsigned long long*>(q.sums) +
                                 ((((int64_t)g * Q + t) * q.H + h) * W + w) * 3 + n;
      atomicAdd(cell, v);
    }
    // (every wave has left step 3 at the barrier above, so the next threshold may overwrite the tables; its two barriers
    //  come before its writes to `red`)
  }
}

bool common_checks_ok(int Q, const int32_t* dir) {
  for (int t = 0; t < Q; ++t)
    if (dir[t] == 0) return false;
  return true;
}

}  // namespace

extern "C" int tecm_event_fss_supported(int32_t rows, int32_t cols) {
  if (rows < 1 || cols < 1) return 0;
  if ((int64_t)rows * cols >= (1 << 24)) return 0;
  return fss_lds_bytes(rows, cols) <= FSS_LDS_MAX ? 1 : 0;
}

extern "C" int tecm_event_hist(const TecmEventHist* e, void* stream) {
  TECM_REQUIRE(e, TECM_E_ARG, "tecm_event_hist: null descriptor");
  TECM_REQUIRE(e->members && e->target && e->thr && e->hist && e->err_flag, TECM_E_ARG, "tecm_event_hist: null pointer");
  TECM_REQUIRE(e->S > 0 && e->H > 0 && e->I > 0 && e->G > 0, TECM_E_ARG, "tecm_event_hist: bad shape");
  TECM_REQUIRE(e->K >= 1 && e->K <= TECM_ENS_MAX_K, TECM_E_ARG, "tecm_event_hist: K = %d outside [1, %d]", (int)e->K,
               TECM_ENS_MAX_K);
  TECM_REQUIRE(e->Q >= 1 && e->Q <= TECM_EVENT_MAX_Q, TECM_E_ARG, "tecm_event_hist: Q = %d outside [1, %d]", (int)e->Q,
               TECM_EVENT_MAX_Q);
  TECM_REQUIRE(common_checks_ok(e->Q, e->dir), TECM_E_ARG, "tecm_event_hist: dir[q] must be non-zero");
  TECM_REQUIRE(e->num_slots >= 1 && (e->slot || e->num_slots == 1), TECM_E_ARG,
               "tecm_event_hist: num_slots must be >= 1, and 1 without a slot tensor");
  const int64_t tiles = (e->I + EV_TILE - 1) / EV_TILE;
  TECM_REQUIRE(e->G <= 65535 && e->H <= 65535, TECM_E_ARG, "tecm_event_hist: G and H must be <= 65535");
  TECM_REQUIRE(tiles < (1 << 24) && tiles * e->H < (1 << 24) && tiles * e->H * e->G < (1 << 24), TECM_E_ARG,
               "tecm_event_hist: more than 2^24 blocks of 64 threads");
  TECM_REQUIRE(e->I <= INT64_MAX / 4 / 2 / (TECM_ENS_MAX_K + 1) / TECM_EVENT_MAX_Q / e->H / e->G, TECM_E_ARG,
               "tecm_event_hist: G * Q * H * (K + 1) * 2 * I counts do not fit 64-bit addressing");
  TECM_REQUIRE(e->scale != 0.0, TECM_E_ARG, "tecm_event_hist: scale must be non-zero");
  TECM_REQUIRE(tecm_aligned(e->members, 4) && tecm_aligned(e->target, 4) && tecm_aligned(e->thr, 4) &&
                   tecm_aligned(e->slot, 4) && tecm_aligned(e->hist, 4) && tecm_aligned(e->group, 4) &&
                   tecm_aligned(e->err_flag, 4),
               TECM_E_ALIGN, "tecm_event_hist: every pointer must be 4-byte aligned");
  const dim3 grid((unsigned)tiles, (unsigned)e->H, (unsigned)e->G);
  const int words = (e->K + 1) * 2 * e->Q;
  if (words <= TECM_EVENT_LDS_WORDS)
    hipLaunchKernelGGL(event_hist_kernel<true>, grid, dim3(EV_TILE), (size_t)words * EV_TILE * sizeof(uint32_t),
                       (hipStream_t)stream, *e);
  else
    hipLaunchKernelGGL(event_hist_kernel<false>, grid, dim3(EV_TILE), 0, (hipStream_t)stream, *e);
  TECM_CHECK_LAUNCH("tecm_event_hist");
  return TECM_OK;
}

extern "C" int tecm_event_fss(const TecmEventFss* e, void* stream) {
  TECM_REQUIRE(e, TECM_E_ARG, "tecm_event_fss: null descriptor");
  TECM_REQUIRE(e->pred && e->target && e->thr && e->sums && e->err_flag, TECM_E_ARG, "tecm_event_fss: null pointer");
  TECM_REQUIRE(e->S > 0 && e->H > 0 && e->I > 0 && e->G > 0 && e->rows > 0 && e->cols > 0, TECM_E_ARG,
               "tecm_event_fss: bad shape");
  TECM_REQUIRE((int64_t)e->rows * e->cols == e->I, TECM_E_ARG, "tecm_event_fss: I = %lld is not rows * cols = %d * %d",
               (long long)e->I, (int)e->rows, (int)e->cols);
  TECM_REQUIRE(e->Q >= 1 && e->Q <= TECM_EVENT_MAX_Q, TECM_E_ARG, "tecm_event_fss: Q = %d outside [1, %d]", (int)e->Q,
               TECM_EVENT_MAX_Q);
  TECM_REQUIRE(e->W >= 1 && e->W <= TECM_EVENT_MAX_W, TECM_E_ARG, "tecm_event_fss: W = %d outside [1, %d]", (int)e->W,
               TECM_EVENT_MAX_W);
  for (int w = 0; w < e->W; ++w)
    TECM_REQUIRE(e->widths[w] >= 1 && e->widths[w] <= 127 && (e->widths[w] & 1), TECM_E_ARG,
                 "tecm_event_fss: width %d must be odd and in [1, 127]", (int)e->widths[w]);
  TECM_REQUIRE(common_checks_ok(e->Q, e->dir), TECM_E_ARG, "tecm_event_fss: dir[q] must be non-zero");
  TECM_REQUIRE(e->num_slots >= 1 && (e->slot || e->num_slots == 1), TECM_E_ARG,
               "tecm_event_fss: num_slots must be >= 1, and 1 without a slot tensor");
  TECM_REQUIRE(tecm_event_fss_supported(e->rows, e->cols) == 1, TECM_E_ARG,
               "tecm_event_fss: a %d x %d grid needs %lld B of LDS, more than %lld (tecm_event_fss_supported)", (int)e->rows,
               (int)e->cols, (long long)fss_lds_bytes(e->rows, e->cols), (long long)FSS_LDS_MAX);
  TECM_REQUIRE(e->S <= 65535 && e->H <= 65535 && e->G <= 65535, TECM_E_ARG, "tecm_event_fss: S, H and G must be <= 65535");
  TECM_REQUIRE(e->scale != 0.0, TECM_E_ARG, "tecm_event_fss: scale must be non-zero");
  TECM_REQUIRE(tecm_aligned(e->sums, 8), TECM_E_ALIGN, "tecm_event_fss: sums must be 8-byte aligned");
  TECM_REQUIRE(tecm_aligned(e->pred, 4) && tecm_aligned(e->target, 4) && tecm_aligned(e->thr, 4) && tecm_aligned(e->slot, 4) &&
                   tecm_aligned(e->group, 4) && tecm_aligned(e->err_flag, 4),
               TECM_E_ALIGN, "tecm_event_fss: every pointer must be 4-byte aligned");
  hipLaunchKernelGGL(event_fss_kernel, dim3((unsigned)e->H, (unsigned)e->S), dim3(FSS_THREADS),
                     (size_t)fss_lds_bytes(e->rows, e->cols), (hipStream_t)stream, *e);
  TECM_CHECK_LAUNCH("tecm_event_fss");
  return TECM_OK;
}
