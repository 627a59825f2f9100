"""Thin, typed wrappers over the C ABI (include/tecmollm.h).  Every function launches HIP kernels
asynchronously on torch's current stream; tensors are only used as device-memory handles."""
from __future__ import annotations

import os
import ctypes as C
from typing import List, Optional, Tuple

import torch

from . import _lib
from ._lib import TecmDrop, TecmGemm, TecmWin, check, lib, ptr, stream_ptr

A_MK, A_KM = 0, 1
B_NK, B_KN = 0, 1
ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH = 0, 1, 2

_MASK64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _MASK64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def win(N: int, Lin: int, Lout: int, stride_t: int, taps: int, Cw: int, pad: int) -> TecmWin:
    return TecmWin(1, N, Lin, Lout, stride_t, taps, Cw, pad)


NO_WIN = TecmWin(0, 0, 0, 0, 0, 0, 0, 0)


# The step's dropout word (TecmDrop::seed_dev): a device uint64 every mask-drawing kernel adds to its recorded seed.  None
# outside a captured step (tecmollm/train.py: TrainStep.step_graphed sets it while it records and replays).
SEED_WORD: Optional[torch.Tensor] = None


def drop(p: float, seed: int, ld: int) -> TecmDrop:
    return TecmDrop(float(p), 0, seed & _MASK64, int(ld), SEED_WORD.data_ptr() if SEED_WORD is not None else None)


NO_DROP = TecmDrop(0.0, 0, 0, 0, None)


def _off(t: torch.Tensor, col_off: int = 0) -> int:
    return t.data_ptr() + t.element_size() * col_off


def gemm(M: int, N: int, K: int, A: torch.Tensor, lda: int, B: torch.Tensor, ldb: int, Cout: torch.Tensor, ldc: int,
         *, a_layout: int = A_MK, b_layout: int = B_NK, a_off: int = 0, b_off: int = 0, c_off: int = 0,
         a_win: Optional[TecmWin] = None, b_win: Optional[TecmWin] = None, c_win: Optional[TecmWin] = None,
         a_drop: Optional[TecmDrop] = None, b_drop: Optional[TecmDrop] = None, out_drop: Optional[TecmDrop] = None,
         alpha: float = 1.0, act: int = ACT_NONE, bias: Optional[torch.Tensor] = None,
         rowbias: Optional[Tuple[torch.Tensor, int, int, int]] = None,
         preact: Optional[Tuple[torch.Tensor, int]] = None, dact_src: Optional[Tuple[torch.Tensor, int]] = None,
         residual: Optional[Tuple[torch.Tensor, int]] = None, accumulate: bool = False, split_k: int = 1,
         bf16: bool = False, dead_rect: Optional[Tuple[int, int, int]] = None,
         zero_rect: Optional[Tuple[int, int, int]] = None) -> None:
    # A / B / Cout may be torch.bfloat16 tensors (bf16 mode only, plain MK x NK): operands that already live in HBM as
    # bf16 (activations rounded once by their producer, cached bf16 weights) and / or a bf16 output for such a consumer
    """C[M,N] = epilogue(alpha * A_view[M,K] . B_view[K,N]); see TecmGemm in include/tecmollm.h.
    *_off are element offsets added to the base pointers (column slices of wider buffers).
    dact_src replaces the activation by a multiplication with act'(dact_src); act then names the activation whose
    derivative is taken and must not be ACT_NONE (the library refuses it).
    bf16 is the precision code: 0/False exact fp32, 1/True bf16 matrix cores, 2 bf16x3 (split-bf16, ~1e-5),
    3 bf16x6 (three-way split, fp32-grade).
    bf16=True asks for the bf16 matrix cores (operands rounded to bf16, fp32 accumulate); calls the bf16
    kernel cannot serve (N < 64 output columns or operands that are not 16-byte friendly) run on the exact
    fp32 kernel instead -- the choice is a pure function of shapes/alignment (`uses_bf16`), never silent:
    with timing on, every record carries the name of the kernel the library launched (tecm_gemm_last_kernel).
    dead_rect = (period, rows, cols) and zero_rect = (period, rows, k) are TecmGemm's two hints: elements of C nobody will
    read, and a rectangle of A known to hold zeros.  Promises about the caller's data that a kernel may use or ignore; the
    timing records count the flops the call issued (2 M N K less tecm_gemm_last_skipped_flops)."""
    g = TecmGemm()
    g.M, g.N, g.K = M, N, K
    io = (IO_A_BF16 if A.dtype == torch.bfloat16 else 0) | (IO_B_BF16 if B.dtype == torch.bfloat16 else 0) | \
         (IO_C_BF16 if Cout.dtype == torch.bfloat16 else 0)
    pre_dt = {t[0].dtype for t in (preact, dact_src) if t is not None}     # ONE flag covers both pointers: they must agree
    if len(pre_dt) > 1:
        raise ValueError("gemm: preact and dact_src must share a dtype")
    if pre_dt == {torch.bfloat16}:
        io |= IO_PRE_BF16
    if io:
        if int(bf16) != PREC_BF16:
            raise _lib.TecmError("bf16 tensors are accepted by the bf16 GEMM only")
        g.io_bf16 = io
    g.A, g.lda, g.a_layout = _off(A, a_off), lda, a_layout
    g.B, g.ldb, g.b_layout = _off(B, b_off), ldb, b_layout
    g.C, g.ldc = _off(Cout, c_off), ldc
    g.a_win = a_win or NO_WIN
    g.b_win = b_win or NO_WIN
    g.c_win = c_win or NO_WIN
    g.a_drop = a_drop or NO_DROP
    g.b_drop = b_drop or NO_DROP
    g.out_drop = out_drop or NO_DROP
    g.alpha, g.act = alpha, act
    g.bias = ptr(bias)
    if rowbias is not None:
        rb, rb_ld, rb_div, rb_mod = rowbias
        g.rowbias, g.rb_ld, g.rb_div, g.rb_mod = rb.data_ptr(), rb_ld, rb_div, rb_mod
    if preact is not None:
        g.preact, g.ldp = preact[0].data_ptr(), preact[1]
    if dact_src is not None:
        g.dact_src, g.ldd = dact_src[0].data_ptr(), dact_src[1]
    if residual is not None:
        g.residual, g.ldr = residual[0].data_ptr(), residual[1]
    g.accumulate = 1 if accumulate else 0
    g._p1 = GROUP_M
    if dead_rect is not None:
        g.dead_period, g.dead_rows, g.dead_cols = dead_rect
    if zero_rect is not None:
        g.zero_period, g.zero_rows, g.zero_k = zero_rect
    ws = None
    if split_k > 1:
        ws = torch.empty(split_k * M * N, device=Cout.device, dtype=torch.float32)
        g.split_k, g.workspace = split_k, ws.data_ptr()
    else:
        g.split_k = 1
    mode = int(bf16)                                    # 0 exact fp32, 1 bf16 (autocast semantics), 2 bf16x3
    use16 = mode == PREC_BF16 and (io != 0 or _bf16_ok(g))
    use3 = mode in (PREC_BF16X3, PREC_BF16X6) and _x3_ok(g)
    fn, what = ((lib().tecm_gemm_bf16x6, "tecm_gemm_bf16x6") if (use3 and mode == PREC_BF16X6) else
                (lib().tecm_gemm_bf16x3, "tecm_gemm_bf16x3") if use3 else
                (lib().tecm_gemm_bf16, "tecm_gemm_bf16") if use16 else (lib().tecm_gemm_f32, "tecm_gemm_f32"))
    if _timing is None:
        check(fn(C.byref(g), stream_ptr()), what)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(fn(C.byref(g), stream_ptr()), what)
    e1.record()
    name = lib().tecm_gemm_last_kernel().decode()
    if _timing_detail:
        name += (f" M={M} N={N} K={K} win={g.a_win.enabled}{g.b_win.enabled}{g.c_win.enabled}"
                 f" drop={int(g.a_drop.p > 0)}{int(g.b_drop.p > 0)}{int(g.out_drop.p > 0)} split={g.split_k}"
                 f" act={g.act} acc={g.accumulate} dact={int(dact_src is not None)} res={int(residual is not None)}"
                 f" pre={int(preact is not None)}")
    # algorithmic HBM bytes of the call: every operand / result element once (a windowed operand: its source tensor once)
    ea, eb, ec = A.element_size(), B.element_size(), Cout.element_size()
    nbytes = (min(A.numel(), M * K) if g.a_win.enabled else M * K) * ea + (min(B.numel(), N * K) if g.b_win.enabled else N * K) * eb
    nbytes += M * N * ec * (2 if accumulate else 1)
    for t in (preact, dact_src, residual):
        if t is not None:
            nbytes += M * N * t[0].element_size()
    _timing.append((name, 2.0 * M * N * K - float(lib().tecm_gemm_last_skipped_flops()), e0, e1, float(nbytes)))


PREC_FP32, PREC_BF16, PREC_BF16X3, PREC_BF16X6 = 0, 1, 2, 3
IO_A_BF16, IO_B_BF16, IO_C_BF16, IO_PRE_BF16 = 1, 2, 4, 8       # TecmGemm.io_bf16
GROUP_M = int(os.environ.get("TECM_GROUP_M", "0"))   # m-tiles per L2 super-tile (0 = each kernel's default); tools/ sweep it
BF16_MIN_N = 64


def uses_bf16(N: int, K: int, lda: int, ldb: int, a_layout: int = A_MK, b_layout: int = B_NK, cw_a: int = 4,
              cw_b: int = 4) -> bool:
    """Which GEMMs run on the bf16 matrix cores when bf16 is requested (mirrored by the oracle's emulation)."""
    if N < BF16_MIN_N or lda % 4 or ldb % 4 or cw_a % 4 or cw_b % 4:
        return False
    if a_layout == A_MK and K % 4:
        return False
    return True


def uses_x3(N: int, K: int, lda: int, ldb: int, a_layout: int = A_MK, b_layout: int = B_NK, a_win: bool = False,
            b_win: bool = False, a_drop: bool = False, b_drop: bool = False) -> bool:
    """Which GEMMs the bf16x3 (split-bf16) kernel serves when that mode is requested: the plain MK x NK contraction
    with at least 64 output columns; every other call runs on the exact fp32 kernel."""
    if a_layout != A_MK or b_layout != B_NK or a_win or b_win or a_drop or b_drop:
        return False
    return N >= BF16_MIN_N and lda % 4 == 0 and ldb % 4 == 0 and K % 4 == 0


def _x3_ok(g: TecmGemm) -> bool:
    if not uses_x3(g.N, g.K, g.lda, g.ldb, g.a_layout, g.b_layout, bool(g.a_win.enabled), bool(g.b_win.enabled),
                   g.a_drop.p > 0, g.b_drop.p > 0):
        return False
    return g.A % 16 == 0 and g.B % 16 == 0


def _bf16_ok(g: TecmGemm) -> bool:
    if not uses_bf16(g.N, g.K, g.lda, g.ldb, g.a_layout, g.b_layout, g.a_win.Cw if g.a_win.enabled else 4,
                     g.b_win.Cw if g.b_win.enabled else 4):
        return False
    return g.A % 16 == 0 and g.B % 16 == 0


# ------------------------------------------------------------------ per-launch timing (bench.py roofline)
_timing = None
_timing_detail = False


def enable_gemm_timing(detail: bool = False) -> list:
    """Bracket every GEMM launch with events on the launch stream (torch's current stream).
    detail=True keys the records by shape / view / epilogue flags as well (tools/gemm_breakdown.py)."""
    global _timing, _timing_detail
    _timing = []
    _timing_detail = detail
    return _timing


def disable_gemm_timing() -> None:
    global _timing
    _timing = None


def summarize_gemm_timing(records: list) -> dict:
    torch.cuda.synchronize()
    agg: dict = {}
    for rec in records:
        name, flops, e0, e1 = rec[:4]
        a = agg.setdefault(name, {"ms": 0.0, "flops": 0.0, "n": 0, "bytes": 0.0})
        a["ms"] += e0.elapsed_time(e1)
        a["flops"] += flops
        a["bytes"] += rec[4] if len(rec) > 4 else 0.0
        a["n"] += 1
    return agg


def tn_ok(Mo: int, No: int, K: int) -> bool:
    """Does the natural-orientation bf16 weight-gradient kernel (csrc/gemm_bf16_tn.hip) serve an Mo x No output over K rows?"""
    return os.environ.get("TECM_BF16_TN", "")[:1] != "0" and lib().tecm_gemm_tn_splits(Mo, No, K) >= 2


def pick_split_k(Mo: int, No: int, K: int, target_blocks: int = 512, min_chunk: int = 512,
                 max_splits: int = 256, prec: int = 0) -> int:
    """Split the (huge) reduction dim of a weight-gradient GEMM so the grid fills 256 CUs; capped because every
    split costs one slab of partial sums that the reducer has to read back.  The fp32 kernel has 128 x 128 tiles and
    two blocks per CU; the bf16 kernel (prec = PREC_BF16 and at least 64 output columns) 256 x 128 tiles and ONE block
    per CU, so its grid should be one round of at most 256 blocks, not 270."""
    if int(prec) == PREC_BF16:
        tn = lib().tecm_gemm_tn_splits(Mo, No, K)      # the natural-orientation kernel's own choice for shapes it serves
        if tn >= 2:
            return int(tn)
    if int(prec) == PREC_BF16 and No >= BF16_MIN_N:
        tiles = ((Mo + 255) // 256) * ((No + 127) // 128)
        s = max(1, 256 // max(tiles, 1))
        return int(min(s, max(1, K // min_chunk), max_splits))
    tiles = ((Mo + 127) // 128) * ((No + 127) // 128 if No > 64 else 1)
    s = max(1, target_blocks // max(tiles, 1))
    s = min(s, max(1, K // min_chunk), max_splits)
    return int(s)


def layernorm_fwd(x: torch.Tensor, ldx: int, gamma: torch.Tensor, beta: torch.Tensor, y: Optional[torch.Tensor], ldy: int,
                  stats: torch.Tensor, M: int, D: int, eps: float = 1e-5, y_off: int = 0,
                  y16: Optional[torch.Tensor] = None, ldy16: int = 0, y16d: Optional[torch.Tensor] = None, ldy16d: int = 0,
                  drop16d: Optional[TecmDrop] = None, seq_major: Optional[Tuple[int, int]] = None) -> None:
    """y (fp32) and / or y16 (bf16 copy for a bf16 matrix-core GEMM, BASELINE configs[2]); y16d: a third, optional bf16
    output = dropout(y, drop16d) rounded -- the LoRA branch's input (peft lora_dropout, modules.py:181).  seq_major = (T, N):
    y16d is written sequence-major -- row (b, n, t) for the time-major row (b, t, n) -- the head's view(batch, -1) of ln_f's
    (dropped) output as a plain matrix; drop16d may then be NO_DROP (eval mode).  y16d may also be an fp32 tensor: the dropped
    output unrounded (fp32 mode's head operand), the values dropout_apply makes of y."""
    if y16 is not None and y16.dtype != torch.bfloat16:
        raise _lib.TecmError("layernorm_fwd: y16 must be a bfloat16 tensor")
    if y16d is not None and y16d.dtype not in (torch.bfloat16, torch.float32):
        raise _lib.TecmError("layernorm_fwd: y16d must be a bfloat16 or float32 tensor")
    if y16d is not None and drop16d is None:
        raise _lib.TecmError("layernorm_fwd: y16d needs its dropout spec")
    sT, sN = seq_major if seq_major is not None else (0, 0)
    check(lib().tecm_layernorm_fwd(x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(),
                                   None if y is None else _off(y, y_off), ldy, ptr(y16), ldy16, ptr(y16d), ldy16d,
                                   C.byref(drop16d) if drop16d is not None else None, sT, sN,
                                   1 if (y16d is not None and y16d.dtype == torch.float32) else 0, stats.data_ptr(), M, D, eps, stream_ptr()), "tecm_layernorm_fwd")


def _ln_add(add) -> Optional["_lib.TecmLnAdd"]:
    """add = (dy2 (M, D) fp32 / bf16, ld, drop spec or None)."""
    if add is None:
        return None
    dy2, ld, dspec = add
    if dy2.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.TecmError("layernorm_bwd: dy2 is fp32 or bf16")
    return _lib.TecmLnAdd(dy2=dy2.data_ptr(), ld=ld, bf16=1 if dy2.dtype == torch.bfloat16 else 0,
                          drop=dspec if dspec is not None else NO_DROP)


def layernorm_bwd_blocks(M: int, D: int) -> int:
    nb = C.c_int32(0)
    check(lib().tecm_layernorm_bwd(None, 0, None, 0, None, None, None, None, None, 0, None, None, C.byref(nb), M, D,
                                   None, 0, None, 0, None), "tecm_layernorm_bwd(query)")
    return nb.value


def layernorm_bwd(dy: torch.Tensor, lddy: int, x: torch.Tensor, ldx: int, gamma: torch.Tensor, stats: torch.Tensor,
                  dres: Optional[torch.Tensor], dx: torch.Tensor, M: int, D: int,
                  dx_masked: Optional[torch.Tensor] = None,
                  mask_drop: Optional[TecmDrop] = None, need_dgb: bool = True, add=None, dy_seq_major=None,
                  skip_dx: bool = False, partials_out: Optional[list] = None, dy_seq_fp32: bool = False):
    """dx = dres + LN'(dy); optional dx_masked = dropout(dx, mask_drop) -- fp32, or bf16 when its only reader is a bf16
    GEMM.  dy: fp32 or bf16.  dy_seq_major = (T, N, drop spec or None): dy is the sequence-major matrix (rows (b, n, t), bf16
    or fp32) the head's first Linear returned, still in front of the post-LLM dropout whose mask is applied here.  add =
    (dy2, ld, drop): a second gradient stream of the same tensor, dy += dropmask * dy2 before the LayerNorm backward (the
    LoRA branch's input gradient through lora_dropout's backward).  dy_seq_fp32 declares the sequence-major dy an fp32
    matrix (fp32 mode's head); without it a sequence-major dy must be bf16 -- an upcast copy is refused.  skip_dx: dx_masked is the only output anybody reads --
    the unmasked dx is not stored (the `dx` tensor is left untouched).  Returns (dgamma, dbeta), or (None, None) when
    need_dgb is False (frozen LayerNorm: the per-block partials are not reduced).  partials_out: a list -- the (nb, 2*D)
    partials buffer is appended to it INSTEAD of being reduced (when need_dgb), and (None, None) returned: the caller
    reduces several of them in one launch (colsum_batch) and splits each row into (dgamma, dbeta)."""
    if skip_dx and dx_masked is None:
        raise _lib.TecmError("layernorm_bwd: skip_dx needs dx_masked")
    if dy_seq_major is not None and (dy.dtype == torch.float32) != bool(dy_seq_fp32):
        raise _lib.TecmError("layernorm_bwd: the sequence-major dy is a bf16 matrix, or an fp32 one declared by dy_seq_fp32")
    m16 = 1 if (dx_masked is not None and dx_masked.dtype == torch.bfloat16) else 0
    ad = _ln_add(add)
    dy16 = 1 if dy.dtype == torch.bfloat16 else 0        # bf16 mode: the gradient a bf16 GEMM returned for its input
    nb = layernorm_bwd_blocks(M, D)
    partials = torch.empty(nb, 2 * D, device=dx.device, dtype=torch.float32)
    nbc = C.c_int32(0)
    od = mask_drop if mask_drop is not None else NO_DROP
    dm = None
    if dy_seq_major is not None:
        mT, mN, mdrop = dy_seq_major
        dm = _lib.TecmLnDyMap(T=mT, N=mN, drop=mdrop if mdrop is not None else NO_DROP)
    check(lib().tecm_layernorm_bwd(dy.data_ptr(), lddy, x.data_ptr(), ldx, gamma.data_ptr(), stats.data_ptr(),
                                   ptr(dres), dx.data_ptr(), ptr(dx_masked), m16, C.byref(od), partials.data_ptr(),
                                   C.byref(nbc), M, D, C.byref(ad) if ad is not None else None, dy16,
                                   C.byref(dm) if dm is not None else None, 1 if skip_dx else 0, stream_ptr()),
          "tecm_layernorm_bwd")
    if not need_dgb:
        return None, None
    if partials_out is not None:
        partials_out.append(partials)
        return None, None
    dgb = colsum(partials, 2 * D, nb, 1, 1, 2 * D)
    return dgb[0, :D], dgb[0, D:]


GN_Y_BF16, GN_OUT_BF16, GN_DACT_BF16 = 1, 2, 4


def gn_reg_ok(L: int, N: int, Cout: int) -> bool:
    """True when the register-resident GroupNorm+GELU kernels (csrc/groupnorm.hip: gn_reg_pairs with 4 or 8 waves per
    sequence, at most 9 float4 per lane) serve BOTH directions -- the only kernels that read / write bf16 activations.
    Longer sequences (the reference's default L_in = 336) take the multi-pass fp32 kernels, and the conv block then keeps
    its activations fp32 in bf16 mode too."""
    return lib().tecm_gn_reg_supported(L, N, Cout) == 1


def gn_fwd_path(L: int, N: int, Cout: int, io_bf16: int = 0, act_stride: int = 1) -> str:
    """The kernel groupnorm_gelu_fwd launches for these arguments (io_bf16: GN_* flags) and aligned tensors, with its
    template arguments; "" where the library refuses the call.  Pure host arithmetic."""
    return lib().tecm_gn_fwd_path(L, N, Cout, io_bf16, act_stride).decode()


def gn_bwd_path(L: int, N: int, Cout: int, io_bf16: int = 0, has_seq_sums: Optional[bool] = None) -> str:
    """The same for groupnorm_gelu_bwd.  has_seq_sums: the call hands the library a workspace for the per-sequence sums;
    None: as groupnorm_gelu_bwd does (whenever y is bf16)."""
    if has_seq_sums is None:
        has_seq_sums = bool(io_bf16 & GN_Y_BF16)
    return lib().tecm_gn_bwd_path(L, N, Cout, io_bf16, 1 if has_seq_sums else 0).decode()


def _gn_io(y: torch.Tensor, out: torch.Tensor) -> int:
    if y.dtype == torch.bfloat16:
        if out.dtype != torch.bfloat16:
            raise _lib.TecmError("groupnorm_gelu: a bf16 y comes with bf16 act / dact / dy")
        return GN_Y_BF16 | GN_OUT_BF16
    if y.dtype != torch.float32:
        raise _lib.TecmError("groupnorm_gelu: y is fp32 or bf16")
    return GN_OUT_BF16 if out.dtype == torch.bfloat16 else 0


def gn_y16_ok(L: int, N: int, Cout: int) -> bool:
    """True when the all-bf16 GroupNorm + GELU kernels serve the sequence (the conv block then writes y as bf16)."""
    return os.environ.get("TECM_Y16", "1")[:1] != "0" and lib().tecm_gn_y16_supported(L, N, Cout) == 1


GN_STATS_GIVEN = 8


def groupnorm_gelu_fwd(y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, act: torch.Tensor,
                       stats: torch.Tensor, B: int, L: int, N: int, Cout: int, eps: float = 1e-5, act_stride: int = 1,
                       stats_given: bool = False) -> None:
    """act: fp32, or bf16 in bf16 mode (its dtype says which); y is fp32.  act_stride s > 1: act is the COMPACT
    (B, ceil(L / s), N, 3*Cout) tensor of the time steps t % s == 0 (all the stride-s 1x1 conv behind it reads).
    stats_given (all-bf16 form only): `stats` already holds (mean, rstd) -- conv_fwd(..., stats=) computed them from the y it
    wrote -- and the call is an elementwise pass over the time steps act keeps."""
    La = (L + act_stride - 1) // act_stride
    if act.numel() != B * La * N * 3 * Cout:
        raise _lib.TecmError(f"groupnorm_gelu_fwd: act must hold (B, {La}, N, 3*Cout) values for act_stride {act_stride}")
    io = _gn_io(y, act)
    if stats_given:
        if io != (GN_Y_BF16 | GN_OUT_BF16):
            raise _lib.TecmError("groupnorm_gelu_fwd: given statistics go with a bf16 y and a bf16 act")
        io |= GN_STATS_GIVEN
    check(lib().tecm_groupnorm_gelu_fwd(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), act.data_ptr(),
                                        stats.data_ptr(), B, L, N, Cout, eps, io, act_stride, stream_ptr()),
          "tecm_groupnorm_gelu_fwd")


def groupnorm_gelu_bwd(dact: torch.Tensor, dstride: int, y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                       stats: torch.Tensor, dy: torch.Tensor, B: int, L: int, N: int,
                       Cout: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Returns (dgamma, dbeta, colsum(dy)), each (3*Cout,); the last is the conv-bias gradient.  dact: fp32, or (bf16 mode,
    together with a bf16 dy) the bf16 tensor the strided 1x1 conv's d-input GEMM wrote."""
    nb = C.c_int32(0)
    check(lib().tecm_groupnorm_gelu_bwd(None, dstride, None, None, None, None, None, None, C.byref(nb), B, L, N, Cout,
                                        0, None, None), "tecm_groupnorm_gelu_bwd(query)")
    CT = 3 * Cout
    partials = torch.empty(nb.value, 3 * CT, device=dy.device, dtype=torch.float32)
    io = _gn_io(y, dy)
    if dact.dtype == torch.bfloat16:
        if not io:
            raise _lib.TecmError("groupnorm_gelu_bwd: a bf16 dact comes with a bf16 dy")
        io |= GN_DACT_BF16
    elif io & GN_Y_BF16:
        raise _lib.TecmError("groupnorm_gelu_bwd: a bf16 y comes with a bf16 dact")
    # all-bf16 form: a small workspace for the per-sequence sums lets the library run the two streaming kernels
    sums = torch.empty(B * N * 6, device=dy.device, dtype=torch.float32) if (io & GN_Y_BF16) else None
    check(lib().tecm_groupnorm_gelu_bwd(dact.data_ptr(), dstride, y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                        stats.data_ptr(), dy.data_ptr(), partials.data_ptr(), C.byref(nb), B, L, N,
                                        Cout, io, ptr(sums), stream_ptr()), "tecm_groupnorm_gelu_bwd")
    dgb = colsum(partials, 3 * CT, nb.value, 1, 1, 3 * CT)
    return dgb[0, :CT], dgb[0, CT:2 * CT], dgb[0, 2 * CT:]


ATT_OUT_BF16, ATT_QKV_BF16, ATT_DCTX_BF16 = 1, 2, 4      # io_bf16 of tecm_attention_fwd / _bwd


def attention_fwd(qkv: torch.Tensor, ctx: torch.Tensor, B: int, T: int, N: int, heads: int, D: int,
                  prob_drop: Optional[TecmDrop] = None) -> None:
    pd = prob_drop if prob_drop is not None else NO_DROP
    io = (ATT_OUT_BF16 if ctx.dtype == torch.bfloat16 else 0) | (ATT_QKV_BF16 if qkv.dtype == torch.bfloat16 else 0)
    check(lib().tecm_attention_fwd(qkv.data_ptr(), ctx.data_ptr(), io, B, T, N, heads, D, C.byref(pd), stream_ptr()),
          "tecm_attention_fwd")


def attention_bwd(qkv: torch.Tensor, dctx: torch.Tensor, dqkv: torch.Tensor, B: int, T: int, N: int, heads: int,
                  D: int, prob_drop: Optional[TecmDrop] = None) -> None:
    pd = prob_drop if prob_drop is not None else NO_DROP
    io = (ATT_OUT_BF16 if dqkv.dtype == torch.bfloat16 else 0) | (ATT_QKV_BF16 if qkv.dtype == torch.bfloat16 else 0) | \
        (ATT_DCTX_BF16 if dctx.dtype == torch.bfloat16 else 0)
    check(lib().tecm_attention_bwd(qkv.data_ptr(), dctx.data_ptr(), dqkv.data_ptr(), io, B, T, N, heads, D, C.byref(pd),
                                   stream_ptr()), "tecm_attention_bwd")


def attention_reads_q0(T: int) -> bool:
    """Do the attention kernels for T tokens read the query of token 0?  (No for the compile-time-T instances: that row's
    softmax is 1 and its score gradient 0 whatever q_0 is, so nobody has to compute q_0 and dq_0 is exactly zero.)"""
    return bool(lib().tecm_attention_reads_q0(T))


def temporal_attention_ws_floats(B: int, T: int, N: int, heads: int, D: int, accumulate: bool, matrix: bool = False) -> int:
    """tecm_temporal_attention_ws_floats: floats of workspace the call asks for by default (one chunk of whole windows, at
    most 64 MiB unless one window needs more; 4 for the export alone, which uses none), 0 when the shape is not served.
    Pure host arithmetic."""
    a = _lib.TecmTemporalAttn(B=B, T=T, N=N, heads=heads, D=D, probs=None if accumulate else 8,
                              node_stats=8 if accumulate else None,             # only NULL / non-NULL is read
                              matrix_stats=8 if (accumulate and matrix) else None)
    return int(lib().tecm_temporal_attention_ws_floats(C.byref(a)))


def temporal_attention(qkv: torch.Tensor, B: int, T: int, N: int, heads: int, D: int, *,
                       probs: Optional[torch.Tensor] = None, nodes: Optional[torch.Tensor] = None,
                       node_stats: Optional[torch.Tensor] = None, lag_stats: Optional[torch.Tensor] = None,
                       matrix_stats: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                       groups: Optional[torch.Tensor] = None, layer: int = 0, count: bool = False, err_flag: int = 0,
                       max_ws_bytes: Optional[int] = None) -> None:
    """tecm_temporal_attention (include/tecmollm.h, csrc/attention_probs.hip) on one layer's `qkv` (B*T*N, 3*D), fp32 or bf16,
    as `attention_fwd` reads it.  `probs` (B, Ns, heads, T, T) float32 receives the causal attention probabilities of the
    nodes `nodes` (int32 (Ns), None: all N); `node_stats` (G, Ly, 4, N, heads), `lag_stats` (G, Ly, heads, T), optionally
    `matrix_stats` (G, Ly, heads, T, T) float64 and, with `count`, `counts` (G) int64 are added to at layer slot `layer`, with
    `groups` (B) int32 naming every window's group (an id outside [0, G) skips the window and sets TECM_BAD_GROUP in the error
    word `err_flag` points to; 0: the device's own, `devcheck.error_word`).  `max_ws_bytes` caps the workspace (it must hold one window): the call
    then walks more chunks of windows and returns the same bits."""
    if qkv.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.TecmError(f"qkv must be float32 or bfloat16 (got {qkv.dtype})")
    _lib.require_gpu_tensor(qkv, "qkv", qkv.dtype)
    if qkv.numel() != B * T * N * 3 * D or not qkv.is_contiguous():
        raise ValueError(f"qkv must be a contiguous ({B * T * N}, {3 * D}) tensor, got {tuple(qkv.shape)}")
    Ns = N if nodes is None else int(nodes.numel())
    for name, t, shape, dtype in (("probs", probs, (B, Ns, heads, T, T), torch.float32), ("nodes", nodes, (Ns,), torch.int32),
                                  ("groups", groups, (B,), torch.int32)):
        if t is not None:
            _lib.require_gpu_tensor(t, name, dtype)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {shape} tensor, got {tuple(t.shape)}")
    ng = ly = 0
    if node_stats is not None:
        ng, ly = int(node_stats.shape[0]), int(node_stats.shape[1])
        for name, t, shape, dtype in (("node_stats", node_stats, (ng, ly, 4, N, heads), torch.float64),
                                      ("lag_stats", lag_stats, (ng, ly, heads, T), torch.float64),
                                      ("counts", counts, (ng,), torch.int64)):
            if t is None:
                raise ValueError("the statistics need node_stats, lag_stats and counts together")
            _lib.require_gpu_tensor(t, name, dtype)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {shape} tensor, got {tuple(t.shape)}")
        if matrix_stats is not None:
            _lib.require_gpu_tensor(matrix_stats, "matrix_stats", torch.float64)
            if tuple(matrix_stats.shape) != (ng, ly, heads, T, T) or not matrix_stats.is_contiguous():
                raise ValueError(f"matrix_stats must be a contiguous {(ng, ly, heads, T, T)} tensor")
    elif matrix_stats is not None:
        raise ValueError("matrix_stats needs node_stats, lag_stats and counts")
    if node_stats is not None and not err_flag:
        from . import devcheck                                  # the device's sticky error word (check_device_errors reads it)
        err_flag = devcheck.error_word(qkv.device).ptr()
    flags = (ATT_QKV_BF16 if qkv.dtype == torch.bfloat16 else 0) | (_lib.TECM_TATT_COUNT if count else 0)
    a = _lib.TecmTemporalAttn(qkv=qkv.data_ptr(), probs=ptr(probs), nodes=ptr(nodes), node_stats=ptr(node_stats),
                              lag_stats=ptr(lag_stats), matrix_stats=ptr(matrix_stats), counts=ptr(counts), group=ptr(groups),
                              err_flag=err_flag or None, B=B, T=T, N=N, heads=heads, D=D, Ns=Ns, num_groups=ng,
                              num_layers=ly, layer=int(layer), flags=flags)
    nws = int(lib().tecm_temporal_attention_ws_floats(C.byref(a)))
    ws = None
    if nws > 0 and node_stats is not None:
        if max_ws_bytes is not None:
            nws = min(nws, int(max_ws_bytes) // 4)
        ws = torch.empty(nws, device=qkv.device, dtype=torch.float32)
        a.ws, a.ws_floats = ws.data_ptr(), nws
    check(lib().tecm_temporal_attention(C.byref(a), stream_ptr()), "tecm_temporal_attention")


def colsum(inp: torch.Tensor, ld: int, outer: int, inner: int, nseg: int, Cn: int, *, in_off: int = 0,
           scale: float = 1.0, in_drop: Optional[TecmDrop] = None, out: Optional[torch.Tensor] = None,
           accumulate: bool = False, twin: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[s][c] = scale * sum_{o<outer, j<inner} in[((o*nseg + s)*inner + j)*ld + c]  -> (nseg, Cn).
    twin: a contiguous bf16 (rows, Cn) tensor that receives the (masked) input values from the same pass."""
    if out is None:
        out = torch.empty(nseg, Cn, device=inp.device, dtype=torch.float32)
    ws = torch.empty(1024 * nseg * Cn, device=inp.device, dtype=torch.float32)     # contract: include/tecmollm.h
    idr = in_drop if in_drop is not None else NO_DROP
    if twin is not None and not (Cn % 4 == 0 and Cn <= 1024 and ld % 4 == 0):
        # wider than the one-pass kernel's 256 column quads (the head at L_in = 96: 1152 columns): two passes
        if in_drop is not None or ld != Cn or in_off:
            raise _lib.TecmError("colsum: a bf16 twin of a masked or strided input needs Cn % 4 == 0 and Cn <= 1024")
        cast_bf16(inp, Cn, twin, Cn, outer * nseg * inner, Cn)
        twin = None
    if twin is not None:
        if twin.dtype != torch.bfloat16 or twin.numel() != outer * nseg * inner * Cn:
            raise _lib.TecmError("colsum: twin must be a contiguous bf16 tensor of the input's rows x Cn")
        check(lib().tecm_colsum_twin(_off(inp, in_off), ld, outer, inner, nseg, Cn, out.data_ptr(), Cn, 1 if accumulate else 0,
                                     scale, C.byref(idr), ws.data_ptr(), twin.data_ptr(), Cn, stream_ptr()), "tecm_colsum_twin")
        return out
    check(lib().tecm_colsum(_off(inp, in_off), ld, outer, inner, nseg, Cn, out.data_ptr(), Cn, 1 if accumulate else 0,
                            scale, C.byref(idr), ws.data_ptr(), stream_ptr()), "tecm_colsum")
    return out


def colsum_path(ld: int, outer: int, inner: int, nseg: int, Cn: int, in_misalign_bytes: int = 0, nbuf: int = 0) -> str:
    """The route colsum (nbuf = 0) or colsum_batch (nbuf matrices of `outer` rows) takes -- "v4 rb=1024 chunk=17 waves=16":
    first stage, partial rows per segment, input rows per partial row, waves of the second stage; a batch answers
    "batch ... launches=N" or, where every matrix goes through colsum one by one, "each v4 ..."; "" where the library
    refuses.  in_misalign_bytes: of the input (batch: of its best aligned matrix).  Pure host arithmetic."""
    return lib().tecm_colsum_path(ld, outer, inner, nseg, Cn, in_misalign_bytes, nbuf).decode()


def colsum_batch(mats: List[torch.Tensor], rows: int, Cn: int) -> torch.Tensor:
    """(len(mats), Cn): row i = the column sums of the contiguous (rows, Cn) fp32 matrix mats[i] -- what
    colsum(mats[i], Cn, rows, 1, 1, Cn) returns, bit for bit -- from one native call for all of them."""
    n = len(mats)
    for m in mats:
        if m.dtype != torch.float32 or not m.is_contiguous() or m.numel() != rows * Cn:
            raise _lib.TecmError("colsum_batch: every matrix is a contiguous fp32 (rows, Cn) tensor")
    out = torch.empty(n, Cn, device=mats[0].device, dtype=torch.float32)
    ws = torch.empty(max(1024, 256 * n) * Cn, device=out.device, dtype=torch.float32)     # contract: include/tecmollm.h
    ins = (C.c_void_p * n)(*[m.data_ptr() for m in mats])
    outs = (C.c_void_p * n)(*[out.data_ptr() + 4 * Cn * i for i in range(n)])
    check(lib().tecm_colsum_batch(ins, outs, n, Cn, rows, Cn, ws.data_ptr(), stream_ptr()), "tecm_colsum_batch")
    return out


def cast_bf16(src: torch.Tensor, lds: int, dst: torch.Tensor, ldd: int, rows: int, cols: int, src_off: int = 0,
              dst_off: int = 0) -> None:
    """dst (bf16) [r][dst_off + c] = round(src (fp32) [r][src_off + c]) for c < cols."""
    check(lib().tecm_cast_bf16(src.data_ptr() + 4 * src_off, lds, dst.data_ptr() + 2 * dst_off, ldd, rows, cols,
                               stream_ptr()), "tecm_cast_bf16")


def dropout_apply(src: torch.Tensor, rows: int, cols: int, spec: TecmDrop, ld: Optional[int] = None,
                  out_bf16: bool = False, twin_bf16: bool = False):
    """dropout(src) with the library's counter-based mask (index = row*spec.ld + col) as a new contiguous tensor; out_bf16:
    a bf16 one (the masked value rounded once, for a tensor only bf16 contractions read); twin_bf16: (fp32 result, its bf16
    twin) from one pass."""
    dst = torch.empty_like(src, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    twin = torch.empty_like(src, dtype=torch.bfloat16) if twin_bf16 else None
    ld = cols if ld is None else ld
    check(lib().tecm_dropout_apply(src.data_ptr(), ld, dst.data_ptr(), ld, 1 if out_bf16 else 0, ptr(twin), ld, rows, cols,
                                   C.byref(spec), stream_ptr()), "tecm_dropout_apply")
    return (dst, twin) if twin_bf16 else dst


def weight_bf16(W: torch.Tensor, same: bool = True, transposed: bool = False):
    """(W rounded to bf16 [R][C] or None, W^T rounded to bf16 [C][R] or None) of a contiguous fp32 matrix, one launch."""
    R, Cc = W.shape
    s = torch.empty(R, Cc, device=W.device, dtype=torch.bfloat16) if same else None
    t = torch.empty(Cc, R, device=W.device, dtype=torch.bfloat16) if transposed else None
    check(lib().tecm_weight_bf16(W.data_ptr(), Cc, ptr(s), Cc, ptr(t), R, R, Cc, stream_ptr()), "tecm_weight_bf16")
    return s, t


def bf16_twin(src: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """A bf16 copy of a contiguous fp32 (rows, cols) matrix for bf16 contractions that would round it in their loaders
    anyway (bit-identical) -- the natural-orientation weight-gradient kernel takes its operands by LDS-DMA, bf16 only."""
    dst = torch.empty(src.shape, device=src.device, dtype=torch.bfloat16)
    cast_bf16(src, cols, dst, cols, rows, cols)
    return dst


def huber_fwd_bwd(pred: torch.Tensor, target: torch.Tensor, delta: float = 1.0, grad_scale: float = 1.0,
                  want_grad: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    n = pred.numel()
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    dpred = torch.empty_like(pred) if want_grad else None
    ws = torch.empty(1024, device=pred.device, dtype=torch.float32)
    check(lib().tecm_huber_fwd_bwd(pred.data_ptr(), target.data_ptr(), ptr(dpred), loss.data_ptr(), n, delta,
                                   grad_scale, ws.data_ptr(), stream_ptr()), "tecm_huber_fwd_bwd")
    return loss, dpred


def huber_fwd_bwd_strided(pred: torch.Tensor, target: torch.Tensor, delta: float = 1.0, grad_scale: float = 1.0,
                          want_grad: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """HuberLoss(delta, mean) of pred (B, H, N, 1) against target (same shape), each in its own layout (any strides): no
    contiguous copies.  Returns (loss (1,), dpred with pred's shape AND strides -- or None)."""
    if pred.shape != target.shape or pred.dim() != 4 or pred.shape[3] != 1:
        raise _lib.TecmError("huber_fwd_bwd_strided: pred and target are (B, L_out, N, 1) tensors of one shape")
    _lib.require_gpu_tensor(pred, "pred")
    _lib.require_gpu_tensor(target, "target")
    B, H, N, _ = pred.shape
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    dpred = torch.empty_strided(pred.shape, pred.stride(), device=pred.device, dtype=torch.float32) if want_grad else None
    if want_grad and max(st * (sz - 1) for st, sz in zip(pred.stride(), pred.shape)) + 1 > pred.numel():
        raise _lib.TecmError("huber_fwd_bwd_strided: pred must be a dense (permuted) tensor")
    ws = torch.empty(1024, device=pred.device, dtype=torch.float32)
    ps = (C.c_int64 * 3)(*pred.stride()[:3])
    tst = (C.c_int64 * 3)(*target.stride()[:3])
    check(lib().tecm_huber_fwd_bwd_strided(pred.data_ptr(), ps, target.data_ptr(), tst, ptr(dpred), loss.data_ptr(), B, H, N,
                                           delta, grad_scale, ws.data_ptr(), stream_ptr()), "tecm_huber_fwd_bwd_strided")
    return loss, dpred


def _taus_array(taus):
    ts = [float(t) for t in taus]
    if not 1 <= len(ts) <= _lib.TECM_QUANT_MAX_Q:
        raise ValueError(f"between 1 and {_lib.TECM_QUANT_MAX_Q} quantile levels, got {len(ts)}")
    return (C.c_float * _lib.TECM_QUANT_MAX_Q)(*ts), len(ts)


def pinball_fwd_bwd_strided(pred: torch.Tensor, target: torch.Tensor, taus, grad_scale: float = 1.0,
                            want_grad: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """tecm_pinball_fwd_bwd_strided (include/tecmollm.h (3k)(a)): the mean pinball loss of pred (B, Q, H, N) -- the quantile
    view of the model's output, any strides -- against target (B, H, N) or (B, H, N, 1) at the levels `taus`, each read in
    its own layout.  Returns (loss (1,), dpred with pred's shape AND strides -- or None --, loss_levels (Q,))."""
    if target.dim() == 4 and target.shape[3] == 1:
        target = target[..., 0]
    if pred.dim() != 4 or target.dim() != 3 or (pred.shape[0], pred.shape[2], pred.shape[3]) != tuple(target.shape):
        raise _lib.TecmError(f"pinball_fwd_bwd_strided: pred is (B, Q, H, N) and target (B, H, N), got {tuple(pred.shape)} "
                             f"and {tuple(target.shape)}")
    _lib.require_gpu_tensor(pred, "pred")
    _lib.require_gpu_tensor(target, "target")
    B, Q, H, N = pred.shape
    tarr, nq = _taus_array(taus)
    if nq != Q:
        raise _lib.TecmError(f"pinball_fwd_bwd_strided: {nq} levels for a pred of {Q}")
    if want_grad:
        # dense and non-overlapping: sorted by stride, every dimension of more than one element steps over all the smaller ones
        dims, span = sorted((st, sz) for st, sz in zip(pred.stride(), pred.shape) if sz > 1), 1
        for st, sz in dims:
            if st != span:
                raise _lib.TecmError("pinball_fwd_bwd_strided: pred must be a dense (permuted) tensor without overlap")
            span *= sz
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    levels = torch.empty(Q, device=pred.device, dtype=torch.float32)
    dpred = torch.empty_strided(pred.shape, pred.stride(), device=pred.device, dtype=torch.float32) if want_grad else None
    nbx = min((B * H * N + 255) // 256, _lib.TECM_PINBALL_BLOCK_CAP)
    ws = torch.empty(Q * nbx, device=pred.device, dtype=torch.float64)
    p = _lib.TecmPinball(pred=pred.data_ptr(), p_stride_b=pred.stride(0), p_stride_q=pred.stride(1), p_stride_h=pred.stride(2),
                         p_stride_n=pred.stride(3), target=target.data_ptr(), t_stride_b=target.stride(0),
                         t_stride_h=target.stride(1), t_stride_n=target.stride(2), B=B, Q=Q, H=H, N=N, taus=tarr,
                         grad_scale=float(grad_scale), dpred=ptr(dpred), loss_out=loss.data_ptr(),
                         loss_levels=levels.data_ptr(), workspace=ws.data_ptr())
    check(lib().tecm_pinball_fwd_bwd_strided(C.byref(p), stream_ptr()), "tecm_pinball_fwd_bwd_strided")
    return loss, dpred, levels


def _qshi(t: torch.Tensor, name: str):
    _lib.require_gpu_tensor(t, name)
    if t.dim() != 4:
        raise ValueError(f"{name} must be (Q, S, H, I), got {tuple(t.shape)}")
    return t.data_ptr(), t.stride(0), t.stride(1), t.stride(2), t.stride(3)


def quantile_stats(levels: torch.Tensor, target: Optional[torch.Tensor], taus, stats: Optional[torch.Tensor],
                   counts: Optional[torch.Tensor], *, adjust: Optional[torch.Tensor] = None, mean: float = 0.0,
                   scale: float = 1.0, clip: Optional[Tuple[float, float]] = None, groups: Optional[torch.Tensor] = None,
                   num_groups: int = 1, err_flag: int = 0, out_z: Optional[torch.Tensor] = None) -> None:
    """tecm_quantile_stats (include/tecmollm.h (3k)(b)): one update of `stats` (G, H, 1 + Q + Q // 2, I) float64 and `counts`
    (same shape) int32 (read as unsigned counts) from `levels` (Q, S, H, I) and `target` (S, H, I), float32 views of any
    strides read in place.  `adjust` is a contiguous (1 or G, H, Q, I) float32 tensor added to the sorted levels; `out_z`
    (Q, S, H, I) float32 receives them.  With `target` None only `out_z` is written (G = `num_groups`)."""
    lp, lq, ls, lh, li = _qshi(levels, "levels")
    Q, S, H, I = levels.shape
    tarr, nq = _taus_array(taus)
    if nq != Q:
        raise ValueError(f"{nq} levels for a tensor of {Q}")
    tp, ts, th, ti = _shi(target, (S, H, I), "target")
    G = int(num_groups) if stats is None else stats.shape[0]
    rows = 1 + Q + Q // 2
    if target is not None:
        if stats is None or stats.shape != (G, H, rows, I) or stats.dtype != torch.float64 or not stats.is_contiguous():
            raise ValueError(f"stats must be a contiguous float64 (G, {H}, {rows}, {I}) tensor")
        if counts is None or counts.shape != (G, H, rows, I) or counts.dtype != torch.int32 or not counts.is_contiguous():
            raise ValueError(f"counts must be a contiguous int32 ({G}, {H}, {rows}, {I}) tensor")
        _lib.require_gpu_tensor(stats, "stats", torch.float64)
        _lib.require_gpu_tensor(counts, "counts", torch.int32)
    elif out_z is None:
        raise ValueError("without a target there must be an out_z")
    Ga = 1
    if adjust is not None:
        _lib.require_gpu_tensor(adjust, "adjust")
        Ga = adjust.shape[0]
        if adjust.shape != (Ga, H, Q, I) or not adjust.is_contiguous() or Ga not in (1, G):
            raise ValueError(f"adjust must be a contiguous (1 or {G}, {H}, {Q}, {I}) tensor, got {tuple(adjust.shape)}")
    if groups is not None:
        _lib.require_gpu_tensor(groups, "groups", torch.int32)
        if groups.shape != (S,) or not groups.is_contiguous():
            raise ValueError(f"groups must hold one contiguous id per sample: {tuple(groups.shape)} for {S} samples")
    op, oq, os_, oh, oi = (None, 0, 0, 0, 0)
    if out_z is not None:
        if out_z.shape != (Q, S, H, I):
            raise ValueError(f"out_z must be (Q, S, H, I) = {(Q, S, H, I)}, got {tuple(out_z.shape)}")
        op, oq, os_, oh, oi = _qshi(out_z, "out_z")
    lo, hi = clip if clip is not None else (0.0, 0.0)
    c = _lib.TecmQuantileStats(levels=lp, l_stride_q=lq, l_stride_s=ls, l_stride_h=lh, l_stride_i=li, target=tp, t_stride_s=ts,
                               t_stride_h=th, t_stride_i=ti, S=S, H=H, G=G, I=I, Q=Q, Ga=Ga, taus=tarr, mean=float(mean),
                               scale=float(scale), clip_lo=lo, clip_hi=hi, clip=1 if clip is not None else 0,
                               adjust=ptr(adjust), stats=ptr(stats), counts=ptr(counts), group=ptr(groups),
                               err_flag=err_flag or None, out_z=op, o_stride_q=oq, o_stride_s=os_, o_stride_h=oh,
                               o_stride_i=oi)
    check(lib().tecm_quantile_stats(C.byref(c), stream_ptr()), "tecm_quantile_stats")


def quantile_scores(levels: torch.Tensor, target: torch.Tensor, scores: torch.Tensor, row0: int, lo_idx: int, hi_idx: int, *,
                    mean: float = 0.0, scale: float = 1.0, clip: Optional[Tuple[float, float]] = None) -> None:
    """tecm_quantile_scores (include/tecmollm.h (3k)(c)): E = max(z_lo - y, y - z_hi) of the sorted `levels` (Q, S, H, I)
    against `target` (S, H, I) into rows row0 .. row0 + S - 1 of the row-major float32 store `scores`, as
    `conformal_scores` addresses it."""
    lp, lq, ls, lh, li = _qshi(levels, "levels")
    Q, S, H, I = levels.shape
    tp, ts, th, ti = _shi(target, (S, H, I), "target")
    _lib.require_gpu_tensor(scores, "scores")
    if scores.dim() != 2 or scores.stride(1) != 1 or scores.shape[1] < H * I or not 0 <= row0 <= scores.shape[0] - S:
        raise ValueError(f"scores must be a row-major (rows >= {row0 + S}, columns >= {H * I}) store, got {tuple(scores.shape)}")
    if not 0 <= int(lo_idx) <= int(hi_idx) < Q:
        raise ValueError(f"needs 0 <= lo_idx <= hi_idx < {Q}, got {(lo_idx, hi_idx)}")
    lo, hi = clip if clip is not None else (0.0, 0.0)
    c = _lib.TecmQuantileScores(levels=lp, l_stride_q=lq, l_stride_s=ls, l_stride_h=lh, l_stride_i=li, target=tp, t_stride_s=ts,
                                t_stride_h=th, t_stride_i=ti, S=S, H=H, Q=Q, I=I, lo_idx=int(lo_idx), hi_idx=int(hi_idx),
                                mean=float(mean), scale=float(scale), clip_lo=lo, clip_hi=hi,
                                clip=1 if clip is not None else 0, scores=scores.data_ptr(),
                                ld=scores.stride(0) if scores.shape[0] > 1 else max(scores.stride(0), H * I), row0=int(row0))
    check(lib().tecm_quantile_scores(C.byref(c), stream_ptr()), "tecm_quantile_scores")


def lora_fold(lB: torch.Tensor, scale: float, w_kn: Optional[torch.Tensor], w_nk: Optional[torch.Tensor], k_off: int) -> None:
    """The LoRA rows of [ W ; s B^T ] (w_kn: (k_off + r, n)) and / or the LoRA columns of [ W^T | s B ] (w_nk: (n, k_off + r))
    from lora_B (n, r); either operand fp32 or bf16, in place."""
    n, r = lB.shape
    for w, shape in ((w_kn, (k_off + r, n)), (w_nk, (n, k_off + r))):
        if w is not None and (tuple(w.shape) != shape or not w.is_contiguous() or w.dtype not in (torch.float32, torch.bfloat16)):
            raise _lib.TecmError(f"lora_fold: operand must be a contiguous {shape} fp32 / bf16 tensor")
    check(lib().tecm_lora_fold(lB.data_ptr(), n, r, float(scale), ptr(w_kn), n, int(w_kn is not None and w_kn.dtype == torch.bfloat16),
                               ptr(w_nk), k_off + r, int(w_nk is not None and w_nk.dtype == torch.bfloat16), k_off,
                               stream_ptr()), "tecm_lora_fold")


def pack_vectors(vecs, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch.cat of up to 12 small contiguous fp32 device vectors in ONE launch."""
    vecs = [v.detach() for v in vecs]
    if any(v.dtype != torch.float32 or not v.is_contiguous() or v.dim() != 1 for v in vecs) or not 1 <= len(vecs) <= 12:
        raise _lib.TecmError("pack_vectors: 1..12 contiguous fp32 vectors")
    total = sum(v.numel() for v in vecs)
    if out is None:
        out = torch.empty(total, device=vecs[0].device, dtype=torch.float32)
    srcs = (C.c_void_p * len(vecs))(*[v.data_ptr() for v in vecs])
    lens = (C.c_int32 * len(vecs))(*[v.numel() for v in vecs])
    check(lib().tecm_pack_vectors(srcs, lens, len(vecs), out.data_ptr(), stream_ptr()), "tecm_pack_vectors")
    return out


def conv_weight_pack(w: torch.Tensor, want_bwd: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    Cout, Cin, k = w.shape
    fwd = torch.empty(Cout, k * Cin, device=w.device, dtype=torch.float32)
    bwd = torch.empty(k * Cout, Cin, device=w.device, dtype=torch.float32) if want_bwd else None
    check(lib().tecm_conv_weight_pack(w.data_ptr(), fwd.data_ptr(), ptr(bwd), Cout, Cin, k, stream_ptr()),
          "tecm_conv_weight_pack")
    return fwd, bwd


def conv_weight_unpack(dpack: torch.Tensor, Cout: int, Cin: int, k: int) -> torch.Tensor:
    dw = torch.empty(Cout, Cin, k, device=dpack.device, dtype=torch.float32)
    check(lib().tecm_conv_weight_unpack(dpack.data_ptr(), dw.data_ptr(), Cout, Cin, k, stream_ptr()),
          "tecm_conv_weight_unpack")
    return dw


def conv_dx_seq_ok(Lc: int, Cout: int, ld_in: int, f32: bool = False) -> bool:
    """Shapes the sequence-tile d-input kernel (csrc/conv_seq.hip) serves IN THIS PRECISION -- divisibility and the LDS
    bytes of one tile, asked of the library itself (tecm_conv_dx_supported) so that the two can never disagree; everything
    else takes the window-view GEMMs."""
    return (os.environ.get("TECM_CONV_SEQ", "1")[:1] != "0"
            and lib().tecm_conv_dx_supported(Lc, Cout, ld_in, 1 if f32 else 0) == 1)


def conv_dx(dy: torch.Tensor, w3: torch.Tensor, w5: torch.Tensor, w7: torch.Tensor, dinp: torch.Tensor, B: int,
            Lc: int, N: int, Cout: int, cin: int, ld_in: int) -> None:
    """dinp (B, Lc, N, ld_in) fp32 = input gradient of the three parallel Conv1d of a Multi_Scale_Conv_Block
    (modules.py:43-60) from dy (B, Lc, N, 3*Cout), in one launch that reads dy once (csrc/conv_seq.hip).  dy bf16: the
    bf16 mode's arithmetic (weights rounded to bf16, fp32 accumulate); dy fp32: exact fp32."""
    if dinp.dtype != torch.float32 or dy.dtype not in (torch.bfloat16, torch.float32):
        raise _lib.TecmError("conv_dx: dy is bf16 or fp32, dinp fp32")
    f32 = dy.dtype == torch.float32
    nci = (ld_in + 31) // 32
    wpack = torch.empty(15 * Cout * nci * 32, device=dy.device, dtype=dy.dtype)
    pack, run, what = ((lib().tecm_conv_dx_pack_f32, lib().tecm_conv_dx_f32, "tecm_conv_dx_f32") if f32 else
                       (lib().tecm_conv_dx_pack, lib().tecm_conv_dx_bf16, "tecm_conv_dx_bf16"))
    check(pack(w3.data_ptr(), w5.data_ptr(), w7.data_ptr(), wpack.data_ptr(), Cout, cin, ld_in, stream_ptr()), what + "/pack")
    d = _lib.TecmConvDx(dy=dy.data_ptr(), wpack=wpack.data_ptr(), dinp=dinp.data_ptr(), B=B, Lc=Lc, N=N, Cout=Cout,
                        ld_in=ld_in)
    if _timing is None:
        check(run(C.byref(d), stream_ptr()), what)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(run(C.byref(d), stream_ptr()), what)
    e1.record()
    name = ("conv_dx_seq_f32_kernel" if f32 else "conv_dx_seq_kernel") + \
        (f" M={B * Lc * N} N={ld_in} K={15 * Cout}" if _timing_detail else "")
    _timing.append((name, 2.0 * B * Lc * N * ld_in * 15 * Cout, e0, e1))


conv_dx_bf16 = conv_dx      # round-3 name (tests)


def conv_dw_seq_ok(Lc: int, Cout: int, ld_in: int) -> bool:
    """Shapes the sequence-tile weight-gradient kernel (csrc/conv_dw_seq.hip) serves (tecm_conv_dw_supported)."""
    return os.environ.get("TECM_CONV_DW_SEQ", "1")[:1] != "0" and lib().tecm_conv_dw_supported(Lc, Cout, ld_in) == 1


_cu_count = {}


def conv_dw(inp: torch.Tensor, dy: torch.Tensor, B: int, Lc: int, N: int, Cout: int, cin: int, ld_in: int):
    """(dw3, dw5, dw7), fp32 (Cout, cin, k): weight gradients of the three parallel Conv1d of a Multi_Scale_Conv_Block
    (modules.py:43-60) from the block input (B, Lc, N, ld_in) and dy (B, Lc, N, 3*Cout), in one persistent launch that
    reads both once (csrc/conv_dw_seq.hip) + a fixed-order reduction of the per-block slabs.  Both bf16: the bf16 mode's
    arithmetic; both fp32: exact fp32."""
    if inp.dtype != dy.dtype or dy.dtype not in (torch.bfloat16, torch.float32):
        raise _lib.TecmError("conv_dw: inp and dy are both bf16 or both fp32 tensors")
    f32 = dy.dtype == torch.float32
    run, what = (lib().tecm_conv_dw_f32, "tecm_conv_dw_f32") if f32 else (lib().tecm_conv_dw_bf16, "tecm_conv_dw_bf16")
    dev = dy.device
    nb = _cu_count.get(dev.index)
    if nb is None:
        nb = _cu_count[dev.index] = int(os.environ.get("TECM_CONV_DW_BLOCKS", 0)) or \
            torch.cuda.get_device_properties(dev).multi_processor_count
    nws = lib().tecm_conv_dw_workspace(Cout, ld_in, nb)
    if nws <= 0:
        raise _lib.TecmError(f"conv_dw: no kernel for Cout={Cout}, ld_in={ld_in}")
    ws = torch.empty(nws, device=dev, dtype=torch.float32)
    dws = [torch.empty(Cout, cin, k, device=dev, dtype=torch.float32) for k in (3, 5, 7)]
    d = _lib.TecmConvDw(inp=inp.data_ptr(), dy=dy.data_ptr(), workspace=ws.data_ptr(), dw3=dws[0].data_ptr(),
                        dw5=dws[1].data_ptr(), dw7=dws[2].data_ptr(), B=B, Lc=Lc, N=N, Cout=Cout, Cin=cin, ld_in=ld_in,
                        num_blocks=nb)
    if _timing is None:
        check(run(C.byref(d), stream_ptr()), what)
        return dws
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(run(C.byref(d), stream_ptr()), what)
    e1.record()
    name = ("conv_dw_seq_f32_kernel" if f32 else "conv_dw_seq_kernel") + (f" M={15 * ld_in} N={Cout} K={B * Lc * N}" if _timing_detail else "")
    _timing.append((name, 2.0 * B * Lc * N * ld_in * 15 * Cout, e0, e1))
    return dws


def conv_fwd_seq_ok(Lc: int, Cout: int, ld_in: int, f32: bool = False) -> bool:
    """As conv_dx_seq_ok, for the forward kernel (tecm_conv_fwd_supported: 64 KiB of LDS per tile)."""
    return (os.environ.get("TECM_CONV_SEQ", "1")[:1] != "0" and os.environ.get("TECM_CONV_FWD_SEQ", "1")[:1] != "0"
            and lib().tecm_conv_fwd_supported(Lc, Cout, ld_in, 1 if f32 else 0) == 1)


def conv_fwd_stats_ok(Lc: int) -> bool:
    """conv_fwd can compute the GroupNorm statistics when one tile holds a whole sequence (tecm_conv_fwd_stats_supported)."""
    return os.environ.get("TECM_CONV_STATS", "1")[:1] != "0" and lib().tecm_conv_fwd_stats_supported(Lc) == 1


def conv_fwd(inp: torch.Tensor, w3: torch.Tensor, w5: torch.Tensor, w7: torch.Tensor, bias: torch.Tensor,
             y: torch.Tensor, B: int, Lc: int, N: int, Cout: int, cin: int, ld_in: int,
             stats: Optional[torch.Tensor] = None, eps: float = 1e-5) -> None:
    """y (B, Lc, N, 3*Cout) fp32 = the three parallel Conv1d (k = 3, 5, 7) of a Multi_Scale_Conv_Block (modules.py:43-60)
    of inp (B, Lc, N, ld_in), bias (3*Cout) included, in one launch (csrc/conv_seq.hip).  inp bf16: the bf16 mode's
    arithmetic; inp fp32: exact fp32."""
    if inp.dtype not in (torch.bfloat16, torch.float32) or y.dtype not in (torch.bfloat16, torch.float32) or \
            (y.dtype == torch.bfloat16 and inp.dtype != torch.bfloat16):
        raise _lib.TecmError("conv_fwd: inp is bf16 or fp32, y fp32 (or bf16 next to a bf16 inp)")
    f32 = inp.dtype == torch.float32
    if f32:
        nval = sum(((3 + 2 * j) * ld_in // 8) * (Cout // 32) for j in range(3)) * 256
        pack, run, what = lib().tecm_conv_fwd_pack_f32, lib().tecm_conv_fwd_f32, "tecm_conv_fwd_f32"
    else:
        nval = sum((((3 + 2 * j) * ld_in + 15) // 16) * (Cout // 32) for j in range(3)) * 512
        pack, run, what = lib().tecm_conv_fwd_pack, lib().tecm_conv_fwd_bf16, "tecm_conv_fwd_bf16"
    wpack = torch.empty(nval, device=y.device, dtype=inp.dtype)
    check(pack(w3.data_ptr(), w5.data_ptr(), w7.data_ptr(), wpack.data_ptr(), Cout, cin, ld_in, stream_ptr()), what + "/pack")
    d = _lib.TecmConvFwd(inp=inp.data_ptr(), wpack=wpack.data_ptr(), bias=bias.data_ptr(), y=y.data_ptr(), B=B, Lc=Lc,
                         N=N, Cout=Cout, ld_in=ld_in, y_bf16=1 if y.dtype == torch.bfloat16 else 0,
                         stats=ptr(stats), eps=eps)     # stats: (B*N, 3, 2) GroupNorm(1) mean / rstd of the bf16 y (one tile per sequence)
    if _timing is None:
        check(run(C.byref(d), stream_ptr()), what)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(run(C.byref(d), stream_ptr()), what)
    e1.record()
    name = ("conv_fwd_seq_f32_kernel" if f32 else "conv_fwd_seq_kernel") + \
        (f" M={B * Lc * N} N={3 * Cout} K={5 * ld_in}(avg)" if _timing_detail else "")
    _timing.append((name, 2.0 * B * Lc * N * Cout * 15 * ld_in, e0, e1))


conv_fwd_bf16 = conv_fwd    # round-3 name (tests)


def transpose_scale(src: torch.Tensor, lds: int, dst: torch.Tensor, ldd: int, rows: int, cols: int, scale: float,
                    dst_off: int = 0) -> None:
    """dst[r*ldd + c] = scale * src[c*lds + r]."""
    check(lib().tecm_transpose_scale(src.data_ptr(), lds, _off(dst, dst_off), ldd, rows, cols, scale, stream_ptr()),
          "tecm_transpose_scale")


ENSEMBLE_OUTPUTS = ("mean", "std", "lo", "hi", "mean_raw")


def ensemble_stats(members: torch.Tensor, target: torch.Tensor, stats: torch.Tensor, hist: torch.Tensor, *, trim: int = 0,
                   mean: float = 0.0, scale: float = 1.0, clip: Optional[Tuple[float, float]] = None,
                   groups: Optional[torch.Tensor] = None, err_flag: int = 0,
                   outputs: Optional[dict] = None) -> None:
    """tecm_ensemble_stats (include/tecmollm.h (3c)): one update of `stats` (G, H, 9, I) float64 and `hist` (G, H, K+1, I)
    int32 (read as unsigned counts) from `members` (K, S, H, I) and `target` (S, H, I), float32 views of any strides, read in
    place.  `clip` = (lo, hi) clamps the members after the inverse transform (mean, scale); `groups` (S) int32 or None;
    `err_flag` is the address of the device error word (tecmollm/devcheck.py).  `outputs` maps names of ENSEMBLE_OUTPUTS to
    (S, H, I) float32 tensors that all have the strides of the first one; names left out are not written."""
    K, S, H, I = members.shape
    G = stats.shape[0]
    if target.shape != (S, H, I):
        raise ValueError(f"target must be (S, H, I) = {(S, H, I)}, got {tuple(target.shape)}")
    if stats.shape != (G, H, _lib.TECM_ENS_STATS, I) or stats.dtype != torch.float64 or not stats.is_contiguous():
        raise ValueError(f"stats must be a contiguous float64 (G, {H}, {_lib.TECM_ENS_STATS}, {I}) tensor")
    if hist.shape != (G, H, K + 1, I) or hist.dtype != torch.int32 or not hist.is_contiguous():
        raise ValueError(f"hist must be a contiguous int32 ({G}, {H}, {K + 1}, {I}) tensor")
    outs = dict(outputs or {})
    unknown = set(outs) - set(ENSEMBLE_OUTPUTS)
    if unknown:
        raise ValueError(f"outputs must come from {ENSEMBLE_OUTPUTS}, got {sorted(unknown)}")
    o_strides = (0, 0, 0)
    for name, t in outs.items():
        _lib.require_gpu_tensor(t, name)
        if t.shape != (S, H, I):
            raise ValueError(f"output {name} must be (S, H, I) = {(S, H, I)}, got {tuple(t.shape)}")
        if o_strides == (0, 0, 0):
            o_strides = tuple(t.stride())
        elif tuple(t.stride()) != o_strides:
            raise ValueError("the per-sample outputs must share their strides")
    lo, hi = clip if clip is not None else (0.0, 0.0)
    e = _lib.TecmEnsemble(members=members.data_ptr(), m_stride_k=members.stride(0), m_stride_s=members.stride(1),
                          m_stride_h=members.stride(2), m_stride_i=members.stride(3),
                          target=target.data_ptr(), t_stride_s=target.stride(0), t_stride_h=target.stride(1),
                          t_stride_i=target.stride(2), S=S, H=H, G=G, I=I, K=K, trim=int(trim),
                          mean=float(mean), scale=float(scale), clip_lo=lo, clip_hi=hi, clip=1 if clip is not None else 0,
                          stats=stats.data_ptr(), hist=hist.data_ptr(), group=ptr(groups), err_flag=err_flag or None,
                          out_mean=ptr(outs.get("mean")), out_std=ptr(outs.get("std")), out_lo=ptr(outs.get("lo")),
                          out_hi=ptr(outs.get("hi")), out_mean_raw=ptr(outs.get("mean_raw")),
                          o_stride_s=o_strides[0], o_stride_h=o_strides[1], o_stride_i=o_strides[2])
    check(lib().tecm_ensemble_stats(C.byref(e), stream_ptr()), "tecm_ensemble_stats")


FIELD_ORDERS = {0.5: _lib.TECM_FIELD_ORDER_HALF, 1.0: _lib.TECM_FIELD_ORDER_ONE, 2.0: _lib.TECM_FIELD_ORDER_TWO}


def field_scores_plan(S: int, H: int, I: int, K: int, NB: int) -> Tuple[int, int, int]:
    """tecm_field_scores_plan: (node tile T, LDS bytes, workspace bytes) of one call with these sizes, as the library computes
    them; TecmError with the library's reason for a shape it does not serve.  Host arithmetic only."""
    tile, lds, ws = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    if not lib().tecm_field_scores_plan(int(S), int(H), int(I), int(K), int(NB), C.byref(tile), C.byref(lds), C.byref(ws)):
        raise _lib.TecmError(lib().tecm_last_error().decode("utf-8", "replace"))
    return tile.value, lds.value, ws.value


def field_scores(members: torch.Tensor, target: torch.Tensor, es_stats: torch.Tensor, vs_stats: Optional[torch.Tensor],
                 pair_class: Optional[torch.Tensor], *, order: float = 0.5, mean: float = 0.0, scale: float = 1.0,
                 clip: Optional[Tuple[float, float]] = None, groups: Optional[torch.Tensor] = None, err_flag: int = 0,
                 es_out: Optional[torch.Tensor] = None, vs_out: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tecm_field_scores (include/tecmollm.h (3m)): one update of `es_stats` (G, H, 4) and `vs_stats` (G, H, NB, 5), float64,
    from `members` (K, S, H, I) and `target` (S, H, I), float32 views of any strides, read in place.  `pair_class` is the
    (I, I) uint8 class matrix (None: the energy score only, `vs_stats` is then not used); `order` 0.5, 1 or 2.  `es_out`
    (S, H, 3) and `vs_out` (S, H, NB, 4), float64, take the per-sample sums.  `workspace` is a uint8 device tensor of at
    least the plan's bytes (one is allocated when it is None or too small).  Returns the workspace used."""
    K, S, H, I = members.shape
    G = es_stats.shape[0]
    if target.shape != (S, H, I):
        raise ValueError(f"target must be (S, H, I) = {(S, H, I)}, got {tuple(target.shape)}")
    if float(order) not in FIELD_ORDERS:
        raise ValueError(f"order must be one of {sorted(FIELD_ORDERS)}, got {order}")
    if es_stats.shape != (G, H, _lib.TECM_FIELD_ES_STATS) or es_stats.dtype != torch.float64 or not es_stats.is_contiguous():
        raise ValueError(f"es_stats must be a contiguous float64 (G, {H}, {_lib.TECM_FIELD_ES_STATS}) tensor")
    NB = 0
    if pair_class is not None:
        _lib.require_gpu_tensor(pair_class, "pair_class", torch.uint8)
        if pair_class.shape != (I, I) or not pair_class.is_contiguous():
            raise ValueError(f"pair_class must be a contiguous uint8 ({I}, {I}) tensor, got {tuple(pair_class.shape)}")
        if vs_stats is None or vs_stats.dim() != 4:
            raise ValueError("pair_class needs vs_stats (G, H, NB, 5)")
        NB = vs_stats.shape[2]
        if (vs_stats.shape != (G, H, NB, _lib.TECM_FIELD_VS_STATS) or vs_stats.dtype != torch.float64
                or not vs_stats.is_contiguous()):
            raise ValueError(f"vs_stats must be a contiguous float64 ({G}, {H}, NB, {_lib.TECM_FIELD_VS_STATS}) tensor")
    for name, t, shape in (("es_out", es_out, (S, H, 3)), ("vs_out", vs_out, (S, H, NB, 4))):
        if t is not None:
            _lib.require_gpu_tensor(t, name, torch.float64)
            if t.shape != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous float64 {shape} tensor, got {tuple(t.shape)}")
    need = field_scores_plan(S, H, I, K, NB)[2]
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 8), device=members.device, dtype=torch.uint8)
    lo, hi = clip if clip is not None else (0.0, 0.0)
    f = _lib.TecmFieldScores(members=members.data_ptr(), m_stride_k=members.stride(0), m_stride_s=members.stride(1),
                             m_stride_h=members.stride(2), m_stride_i=members.stride(3),
                             target=target.data_ptr(), t_stride_s=target.stride(0), t_stride_h=target.stride(1),
                             t_stride_i=target.stride(2), S=S, H=H, G=G, I=I, K=K, NB=NB,
                             mean=float(mean), scale=float(scale), clip_lo=lo, clip_hi=hi, clip=1 if clip is not None else 0,
                             order=FIELD_ORDERS[float(order)], pair_class=ptr(pair_class) if NB else None,
                             es_stats=es_stats.data_ptr(), vs_stats=ptr(vs_stats) if NB else None,
                             es_out=ptr(es_out), vs_out=ptr(vs_out) if NB else None, group=ptr(groups),
                             err_flag=err_flag or None, workspace=workspace.data_ptr(),
                             workspace_bytes=workspace.numel() * workspace.element_size())
    check(lib().tecm_field_scores(C.byref(f), stream_ptr()), "tecm_field_scores")
    return workspace


def member_reorder(values: torch.Tensor, template: torch.Tensor, out: torch.Tensor, rows: Optional[torch.Tensor] = None,
                   out_rank: Optional[torch.Tensor] = None, err_flag: int = 0) -> None:
    """tecm_member_reorder (include/tecmollm.h (3n)): `out[k, s, h, i]` = the value of cell (s, h, i) whose position among the
    cell's K `values` is the position of `template[k, s, h, i]` among the cell's K template values.  `values` and `out`
    (K, S, H, I) float32 views of any strides (`out` may be `values` itself); `template` a (K, S, H, I) view, or with `rows`
    (S, K) int32 contiguous a (T, I) series view whose rows `rows[s, k] + h` are the template; `out_rank` a contiguous uint8
    (K, S, H, I) tensor.  `err_flag` is the address of the device error word, needed with `rows`.  Shapes and dtypes are the
    caller's to check (`tecmollm.coherence.reorder_members` does)."""
    K, S, H, I = values.shape
    r = _lib.TecmMemberReorder(values=values.data_ptr(), v_stride_k=values.stride(0), v_stride_s=values.stride(1),
                               v_stride_h=values.stride(2), v_stride_i=values.stride(3),
                               tmpl=template.data_ptr(), out=out.data_ptr(), o_stride_k=out.stride(0),
                               o_stride_s=out.stride(1), o_stride_h=out.stride(2), o_stride_i=out.stride(3),
                               out_rank=ptr(out_rank), S=S, H=H, K=K, I=I, err_flag=err_flag or None)
    if rows is None:
        r.t_stride_k, r.t_stride_s, r.t_stride_h, r.t_stride_i = template.stride()
    else:
        r.rows, r.T, r.t_stride_row, r.t_stride_i = rows.data_ptr(), template.shape[0], template.stride(0), template.stride(1)
    check(lib().tecm_member_reorder(C.byref(r), stream_ptr()), "tecm_member_reorder")


def _event_common(thr: torch.Tensor, thr_strides, dirs, slots, num_slots: int, S: int, H: int):
    _lib.require_gpu_tensor(thr, "thresholds", torch.float32)
    Q = len(dirs)
    if len(thr_strides) != 3 or min(int(v) for v in thr_strides) < 0:
        raise ValueError(f"thr_strides must be three non-negative element strides (q, slot, node), got {thr_strides}")
    if slots is not None:
        _lib.require_gpu_tensor(slots, "slots", torch.int32)
        if slots.shape != (S, H) or not slots.is_contiguous():
            raise ValueError(f"slots must be a contiguous int32 ({S}, {H}) tensor, got {tuple(slots.shape)}")
    elif int(num_slots) != 1:
        raise ValueError("num_slots must be 1 without a slot tensor")
    d = (C.c_int32 * 8)(*[int(v) for v in list(dirs)[:8]])
    return Q, d


def event_hist(members: torch.Tensor, target: torch.Tensor, hist: torch.Tensor, thr: torch.Tensor, thr_strides, dirs, *,
               slots: Optional[torch.Tensor] = None, num_slots: int = 1, mean: float = 0.0, scale: float = 1.0,
               clip: Optional[Tuple[float, float]] = None, groups: Optional[torch.Tensor] = None, err_flag: int = 0) -> None:
    """tecm_event_hist (include/tecmollm.h (3j a)): one update of `hist` (G, Q, H, K+1, 2, I) int32 (read as unsigned counts)
    from `members` (K, S, H, I) and `target` (S, H, I), float32 views of any strides, read in place.  `thr` is a float32
    device tensor addressed with the element strides `thr_strides` = (q, slot, node), any of which may be 0; `dirs` holds
    one non-zero int per threshold (> 0: above, < 0: below); `slots` (S, H) int32 or None."""
    K, S, H, I = members.shape
    if target.shape != (S, H, I):
        raise ValueError(f"target must be (S, H, I) = {(S, H, I)}, got {tuple(target.shape)}")
    Q, d = _event_common(thr, thr_strides, dirs, slots, num_slots, S, H)
    G = hist.shape[0]
    if hist.shape != (G, Q, H, K + 1, 2, I) or hist.dtype != torch.int32 or not hist.is_contiguous():
        raise ValueError(f"hist must be a contiguous int32 (G, {Q}, {H}, {K + 1}, 2, {I}) tensor")
    lo, hi = clip if clip is not None else (0.0, 0.0)
    e = _lib.TecmEventHist(members=members.data_ptr(), m_stride_k=members.stride(0), m_stride_s=members.stride(1),
                           m_stride_h=members.stride(2), m_stride_i=members.stride(3),
                           target=target.data_ptr(), t_stride_s=target.stride(0), t_stride_h=target.stride(1),
                           t_stride_i=target.stride(2), S=S, H=H, G=G, I=I, K=K, Q=Q, mean=float(mean), scale=float(scale),
                           clip_lo=lo, clip_hi=hi, clip=1 if clip is not None else 0, num_slots=int(num_slots),
                           thr=thr.data_ptr(), th_stride_q=int(thr_strides[0]), th_stride_k=int(thr_strides[1]),
                           th_stride_i=int(thr_strides[2]), slot=ptr(slots), dir=d, hist=hist.data_ptr(),
                           group=ptr(groups), err_flag=err_flag or None)
    check(lib().tecm_event_hist(C.byref(e), stream_ptr()), "tecm_event_hist")


def event_fss_ok(rows: int, cols: int) -> bool:
    """Whether tecm_event_fss serves a rows x cols grid (tecm_event_fss_supported: its LDS map in 64 KiB)."""
    return lib().tecm_event_fss_supported(int(rows), int(cols)) == 1


def event_fss(pred: torch.Tensor, target: torch.Tensor, sums: torch.Tensor, thr: torch.Tensor, thr_strides, dirs, widths,
              grid, *, slots: Optional[torch.Tensor] = None, num_slots: int = 1, mean: float = 0.0, scale: float = 1.0,
              clip: Optional[Tuple[float, float]] = None, groups: Optional[torch.Tensor] = None, err_flag: int = 0) -> None:
    """tecm_event_fss (include/tecmollm.h (3j b)): one update of `sums` (G, Q, H, W, 3) int64 (read as unsigned sums) from a
    deterministic forecast `pred` and `target`, (S, H, I) float32 views read in place, on the (rows, cols) `grid` with
    I == rows * cols, for the odd window `widths`.  Thresholds, directions and slots as in `event_hist`."""
    S, H, I = pred.shape
    if target.shape != (S, H, I):
        raise ValueError(f"target must be (S, H, I) = {(S, H, I)}, got {tuple(target.shape)}")
    Q, d = _event_common(thr, thr_strides, dirs, slots, num_slots, S, H)
    W, G = len(widths), sums.shape[0]
    if sums.shape != (G, Q, H, W, 3) or sums.dtype != torch.int64 or not sums.is_contiguous():
        raise ValueError(f"sums must be a contiguous int64 (G, {Q}, {H}, {W}, 3) tensor")
    wd = (C.c_int32 * 8)(*[int(v) for v in list(widths)[:8]])
    lo, hi = clip if clip is not None else (0.0, 0.0)
    e = _lib.TecmEventFss(pred=pred.data_ptr(), p_stride_s=pred.stride(0), p_stride_h=pred.stride(1),
                          p_stride_i=pred.stride(2), target=target.data_ptr(), t_stride_s=target.stride(0),
                          t_stride_h=target.stride(1), t_stride_i=target.stride(2), S=S, H=H, G=G, I=I, rows=int(grid[0]),
                          cols=int(grid[1]), Q=Q, W=W, mean=float(mean), scale=float(scale), clip_lo=lo, clip_hi=hi,
                          clip=1 if clip is not None else 0, num_slots=int(num_slots), thr=thr.data_ptr(),
                          th_stride_q=int(thr_strides[0]), th_stride_k=int(thr_strides[1]), th_stride_i=int(thr_strides[2]),
                          slot=ptr(slots), dir=d, widths=wd, sums=sums.data_ptr(), group=ptr(groups),
                          err_flag=err_flag or None)
    check(lib().tecm_event_fss(C.byref(e), stream_ptr()), "tecm_event_fss")


CONFORMAL_MODES = {"absolute": _lib.TECM_CONF_ABS, "signed": _lib.TECM_CONF_SIGNED}
INTERVAL_OUTPUTS = ("lo", "hi", "mid")


def _conformal_mode(mode) -> int:
    if mode not in CONFORMAL_MODES:
        raise ValueError(f"mode must be one of {sorted(CONFORMAL_MODES)}, got {mode!r}")
    return CONFORMAL_MODES[mode]


def _shi(t: Optional[torch.Tensor], shape, name: str):
    """(pointer, stride_s, stride_h, stride_i) of an (S, H, I) float32 device view; (None, 0, 0, 0) for None."""
    if t is None:
        return None, 0, 0, 0
    _lib.require_gpu_tensor(t, name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be (S, H, I) = {tuple(shape)}, got {tuple(t.shape)}")
    return t.data_ptr(), t.stride(0), t.stride(1), t.stride(2)


def conformal_scores(pred: torch.Tensor, target: torch.Tensor, scores: torch.Tensor, row0: int = 0, *,
                     mode: str = "absolute", sigma: Optional[torch.Tensor] = None, sigma_min: float = 1e-3,
                     mean: float = 0.0, scale: float = 1.0, clip: Optional[Tuple[float, float]] = None) -> None:
    """tecm_conformal_scores (include/tecmollm.h (3g)(a)): the scores of `pred` against `target`, (S, H, I) float32 views of
    any strides read in place, into rows row0 .. row0 + S - 1 of the 2-D float32 store `scores` (rows of H*I values, leading
    dimension scores.stride(0)).  `sigma` (S, H, I) in physical units divides the score by max(sigma, sigma_min)."""
    S, H, I = pred.shape
    pp, ps, ph, pi = _shi(pred, (S, H, I), "pred")
    tp, ts, th, ti = _shi(target, (S, H, I), "target")
    gp, gs, gh, gi = _shi(sigma, (S, H, I), "sigma")
    _lib.require_gpu_tensor(scores, "scores")
    if scores.dim() != 2 or scores.stride(1) != 1 or scores.shape[1] < H * I or not 0 <= row0 <= scores.shape[0] - S:
        raise ValueError(f"scores must be a row-major (rows >= {row0 + S}, columns >= {H * I}) store, got {tuple(scores.shape)}")
    lo, hi = clip if clip is not None else (0.0, 0.0)
    c = _lib.TecmConformalScores(pred=pp, p_stride_s=ps, p_stride_h=ph, p_stride_i=pi, target=tp, t_stride_s=ts,
                                 t_stride_h=th, t_stride_i=ti, sigma=gp, g_stride_s=gs, g_stride_h=gh, g_stride_i=gi,
                                 S=S, H=H, mode=_conformal_mode(mode), I=I, mean=float(mean), scale=float(scale),
                                 clip_lo=lo, clip_hi=hi, clip=1 if clip is not None else 0, sigma_min=float(sigma_min),
                                 scores=scores.data_ptr(), ld=scores.stride(0), row0=int(row0))
    check(lib().tecm_conformal_scores(C.byref(c), stream_ptr()), "tecm_conformal_scores")


def column_select(x: torch.Tensor, ranks: torch.Tensor, groups: Optional[torch.Tensor] = None, err_flag: int = 0,
                  columns: Optional[int] = None) -> torch.Tensor:
    """tecm_column_select (include/tecmollm.h (3g)(b)): the ranks[g, q]-th smallest (1-based) of every column of the rows of
    group g of `x`, a 2-D float32 device tensor with contiguous rows (any leading dimension; `columns` limits the search to
    the first so many columns).  `ranks` (G, Q) int32 on the device, `groups` (S) int32 on the device or None (one group),
    `err_flag` the address of the device error word (tecmollm/devcheck.py).  Returns (Q, G, C) float32: -inf for a rank
    <= 0, +inf for a rank above the group's row count, numpy's sort order otherwise (NaN last)."""
    _lib.require_gpu_tensor(x, "x")
    _lib.require_gpu_tensor(ranks, "ranks", torch.int32)
    if x.dim() != 2 or x.stride(1) != 1 and x.shape[1] > 1:
        raise ValueError("x must be a 2-D tensor with contiguous rows")
    S, Cn = x.shape[0], int(x.shape[1] if columns is None else columns)
    if ranks.dim() != 2 or not ranks.is_contiguous():
        raise ValueError("ranks must be a contiguous (G, Q) tensor")
    if not 0 < Cn <= x.shape[1]:
        raise ValueError(f"columns must lie in (0, {x.shape[1]}], got {Cn}")
    G, Q = ranks.shape
    if groups is not None:
        _lib.require_gpu_tensor(groups, "groups", torch.int32)
        if groups.shape != (S,) or not groups.is_contiguous():
            raise ValueError(f"groups must hold one contiguous id per row: {tuple(groups.shape)} for {S} rows")
    out = torch.empty(Q, G, Cn, device=x.device, dtype=torch.float32)
    c = _lib.TecmColumnSelect(x=x.data_ptr(), ld=x.stride(0) if S > 1 else max(x.stride(0), Cn), S=S, C=Cn, group=ptr(groups),
                              ranks=ranks.data_ptr(), G=G, Q=Q, out=out.data_ptr(), err_flag=err_flag or None)
    check(lib().tecm_column_select(C.byref(c), stream_ptr()), "tecm_column_select")
    return out


def interval_stats(pred: torch.Tensor, target: Optional[torch.Tensor], q_lo: Optional[torch.Tensor], q_hi: torch.Tensor,
                   stats: Optional[torch.Tensor], *, alpha: float = 0.1, mode: str = "absolute",
                   sigma: Optional[torch.Tensor] = None, sigma_min: float = 1e-3, mean: float = 0.0, scale: float = 1.0,
                   clip: Optional[Tuple[float, float]] = None, groups: Optional[torch.Tensor] = None, num_groups: int = 1,
                   err_flag: int = 0, outputs: Optional[dict] = None) -> None:
    """tecm_interval_stats (include/tecmollm.h (3g)(c)): one update of `stats` (G, H, 6, I) float64 from `pred`, `target`
    (S, H, I) float32 views read in place and the quantiles `q_lo` (None in the absolute mode), `q_hi`, contiguous (Gq, H, I)
    float32 with Gq = 1 or G.  `outputs` maps names of INTERVAL_OUTPUTS to (S, H, I) float32 tensors that share their strides.
    With `target` None only the outputs are written and `stats` may be None (G = `num_groups`)."""
    S, H, I = pred.shape
    pp, ps, ph, pi = _shi(pred, (S, H, I), "pred")
    tp, ts, th, ti = _shi(target, (S, H, I), "target")
    gp, gs, gh, gi = _shi(sigma, (S, H, I), "sigma")
    G = int(num_groups) if stats is None else stats.shape[0]
    if stats is not None and (stats.shape != (G, H, _lib.TECM_INTERVAL_STATS, I) or stats.dtype != torch.float64
                              or not stats.is_contiguous()):
        raise ValueError(f"stats must be a contiguous float64 (G, {H}, {_lib.TECM_INTERVAL_STATS}, {I}) tensor")
    m = _conformal_mode(mode)
    Gq = q_hi.shape[0]
    for name, t in (("q_lo", q_lo), ("q_hi", q_hi)):
        if t is None:
            continue
        _lib.require_gpu_tensor(t, name)
        if t.shape != (Gq, H, I) or not t.is_contiguous() or Gq not in (1, G):
            raise ValueError(f"{name} must be a contiguous (1 or {G}, {H}, {I}) tensor, got {tuple(t.shape)}")
    if (q_lo is None) != (m == _lib.TECM_CONF_ABS):
        raise ValueError("q_lo is given in the signed mode and only there")
    if groups is not None:
        _lib.require_gpu_tensor(groups, "groups", torch.int32)
        if groups.shape != (S,) or not groups.is_contiguous():
            raise ValueError(f"groups must hold one contiguous id per sample: {tuple(groups.shape)} for {S} samples")
    outs = dict(outputs or {})
    unknown = set(outs) - set(INTERVAL_OUTPUTS)
    if unknown:
        raise ValueError(f"outputs must come from {INTERVAL_OUTPUTS}, got {sorted(unknown)}")
    o_strides = (0, 0, 0)
    for name, t in outs.items():
        _lib.require_gpu_tensor(t, name)
        if t.shape != (S, H, I):
            raise ValueError(f"output {name} must be (S, H, I) = {(S, H, I)}, got {tuple(t.shape)}")
        if o_strides == (0, 0, 0):
            o_strides = tuple(t.stride())
        elif tuple(t.stride()) != o_strides:
            raise ValueError("the per-sample outputs must share their strides")
    lo, hi = clip if clip is not None else (0.0, 0.0)
    c = _lib.TecmIntervalStats(pred=pp, p_stride_s=ps, p_stride_h=ph, p_stride_i=pi, target=tp, t_stride_s=ts, t_stride_h=th,
                               t_stride_i=ti, sigma=gp, g_stride_s=gs, g_stride_h=gh, g_stride_i=gi, S=S, H=H, mode=m, I=I,
                               mean=float(mean), scale=float(scale), clip_lo=lo, clip_hi=hi,
                               clip=1 if clip is not None else 0, sigma_min=float(sigma_min), q_lo=ptr(q_lo),
                               q_hi=q_hi.data_ptr(), Gq=Gq, G=G, alpha=float(alpha), stats=ptr(stats), group=ptr(groups),
                               err_flag=err_flag or None, out_lo=ptr(outs.get("lo")), out_hi=ptr(outs.get("hi")),
                               out_mid=ptr(outs.get("mid")), o_stride_s=o_strides[0], o_stride_h=o_strides[1],
                               o_stride_i=o_strides[2])
    check(lib().tecm_interval_stats(C.byref(c), stream_ptr()), "tecm_interval_stats")


def spatial_attention_ws_floats(d: "_lib.TecmSpatial", num_edges: int, accumulate: bool) -> int:
    """tecm_spatial_attention_ws_floats: floats of workspace the call asks for by default (one chunk of graphs, at most
    64 MiB unless one graph needs more), 0 when the descriptor is not served.  Pure host arithmetic."""
    a = _lib.TecmSpatialAttn(E=int(num_edges), edge_stats=8 if accumulate else None)   # only NULL / non-NULL is read
    return int(lib().tecm_spatial_attention_ws_floats(C.byref(d), C.byref(a)))


def spatial_attention(d: "_lib.TecmSpatial", num_edges: int, *, alpha: Optional[torch.Tensor] = None,
                      perm: Optional[torch.Tensor] = None, edge_stats: Optional[torch.Tensor] = None,
                      node_stats: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                      groups: Optional[torch.Tensor] = None, skip_unconnected: bool = False,
                      max_ws_bytes: Optional[int] = None) -> None:
    """tecm_spatial_attention (include/tecmollm.h, csrc/spatial_attn.hip) for the spatial descriptor `d` a forward would run
    with and the `num_edges` = E' entries of its by-target CSR.  `alpha` (B*L, E'' = E' + N, H) float32 receives the
    coefficients, entry q of the CSR at position perm[q] (int32 (E'), None: q), the self loops behind them; `edge_stats`
    (G, 3, E'', H), `node_stats` (G, N, H) float64 and `counts` (G) int64 are added to, in kernel order, with `groups` (B*L)
    int32 naming every graph's group.  `max_ws_bytes` caps the workspace (it must hold one graph): the call then walks
    more chunks of graphs and returns the same bits."""
    G_, N, H = d.B * d.L, d.N, d.H
    E2 = int(num_edges) + N
    dev = torch.device("cuda", torch.cuda.current_device())
    for name, t, shape, dtype in (("alpha", alpha, (G_, E2, H), torch.float32), ("perm", perm, (int(num_edges),), torch.int32),
                                  ("groups", groups, (G_,), torch.int32)):
        if t is not None:
            _lib.require_gpu_tensor(t, name, dtype)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {shape} tensor, got {tuple(t.shape)}")
            dev = t.device
    ng = 0
    if edge_stats is not None:
        ng = edge_stats.shape[0]
        for name, t, shape, dtype in (("edge_stats", edge_stats, (ng, 3, E2, H), torch.float64),
                                      ("node_stats", node_stats, (ng, N, H), torch.float64),
                                      ("counts", counts, (ng,), torch.int64)):
            if t is None:
                raise ValueError("the statistics need edge_stats, node_stats and counts together")
            _lib.require_gpu_tensor(t, name, dtype)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {shape} tensor, got {tuple(t.shape)}")
        dev = edge_stats.device
    nws = spatial_attention_ws_floats(d, num_edges, edge_stats is not None)
    if nws <= 0:
        raise _lib.TecmError("spatial_attention: serves 22 channels in 2 heads: the fused stage with C_in 6 or 10 and "
                             f"d_emb = 22 - C_in, or the stand-alone GATv2 on 22 channels (got C_in = {d.Cin}, d_emb = {d.Demb}, "
                             f"heads = {d.H})")
    if max_ws_bytes is not None:
        nws = min(nws, int(max_ws_bytes) // 4)
    ws = torch.empty(nws, device=dev, dtype=torch.float32)
    a = _lib.TecmSpatialAttn(alpha=ptr(alpha), perm=ptr(perm), edge_stats=ptr(edge_stats), node_stats=ptr(node_stats),
                             counts=ptr(counts), group=ptr(groups), ws=ws.data_ptr(), ws_floats=nws, num_groups=ng,
                             E=int(num_edges), flags=_lib.TECM_ATTN_SKIP_UNCONNECTED if skip_unconnected else 0)
    check(lib().tecm_spatial_attention(C.byref(d), C.byref(a), stream_ptr()), "tecm_spatial_attention")
