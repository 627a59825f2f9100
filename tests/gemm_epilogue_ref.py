"""The epilogue contract of TecmGemm (include/tecmollm.h), stated once in plain torch.

`epilogue_ref` takes the product P = A_view . B_view and the keyword arguments of `ops.gemm` that shape the epilogue, and
returns the C buffer the call must leave behind (and the pre-activation it must store).  It is written in the order the
kernels implement:

    v  = alpha * P + bias[n] + rowbias[(m // rb_div) % rb_mod][n]
    preact[m][n] = v            a bf16 preact stores bf16(v), and v continues as float(bf16(v))
    v  = v * act'(dact_src[m][n])   if dact_src   (act names the activation whose derivative is taken; never act itself)
         act(v)                     otherwise
    v *= keep(seed + word, row * ld + col) / (1 - p)        row, col: the element of C that is stored (under c_win the
                                                            target row and column of the view)
    v += residual[m][n]
    v += previous C[row][col]   if accumulate
    C[row][col] = v             through c_win when enabled (an element whose t_in is outside [0, Lin) is dropped),
                                rounded to bf16 for a bf16 C

Everything else of the buffer -- pad columns ldc > N, target rows no window row maps to -- keeps its previous contents:
the expected buffer starts as a copy of the pre-filled one.  The only library code used is the NumPy mirror of the
dropout hash, `tecmollm.rng.keep_mult`.  `dtype=torch.float32` evaluates the same statement in fp32 (the host test uses
it to show that correct fp32 arithmetic meets the bars the GPU kernels are held to)."""
import functools
import math

import numpy as np
import torch

ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH = 0, 1, 2
_MASK64 = (1 << 64) - 1
_K0 = math.sqrt(2.0 / math.pi)
_K1 = 0.044715


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(_K0 * (x + _K1 * x * x * x)))


def dgelu_tanh(x):
    t = torch.tanh(_K0 * (x + _K1 * x * x * x))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _K0 * (1.0 + 3.0 * _K1 * x * x)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu_erf(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


_ACT = {ACT_GELU_ERF: (gelu_erf, dgelu_erf), ACT_GELU_TANH: (gelu_tanh, dgelu_tanh)}


def round_bf16(x):
    """Round to nearest-even bf16, returned in x's dtype."""
    return x.float().bfloat16().to(x.dtype)


def _view2d(t, ld, M, N, dtype):
    """(tensor, ld) as ops.gemm takes it -> its logical (M, N) block."""
    return t.detach().cpu().reshape(-1)[: M * ld].view(M, ld)[:, :N].to(dtype)


@functools.lru_cache(maxsize=None)
def targets(M, N, c_win=None):
    """Row and column of C that logical element (m, n) is stored at, and whether it is stored at all.
    c_win = (nodes, Lin, Lout, stride_t, taps, Cw, pad): row m = (bq * Lout + t_out) * nodes + node, column n = tap * Cw + c
    goes to row (bq * Lin + t_in) * nodes + node, column c with t_in = t_out * stride_t + tap - pad.
    (The three tensors are cached per geometry and shared: read them, never write them.)"""
    m = torch.arange(M, dtype=torch.int64)[:, None].expand(M, N)
    n = torch.arange(N, dtype=torch.int64)[None, :].expand(M, N)
    if c_win is None:
        return m, n, torch.ones(M, N, dtype=torch.bool)
    nodes, Lin, Lout, stride_t, taps, Cw, pad = c_win
    assert taps * Cw == N
    q, node = m // nodes, m % nodes
    bq, t_out = q // Lout, q % Lout
    tap, c = n // Cw, n % Cw
    t_in = t_out * stride_t + tap - pad
    return (bq * Lin + t_in) * nodes + node, c, (t_in >= 0) & (t_in < Lin)


_masks = {}


def keep_mask(p, seed, ld, seed_word, rows, cols, key):
    """keep / (1 - p) per element, drawn once per (seed + word, p, ld, index geometry `key`) and reused."""
    from tecmollm.rng import keep_mult
    seed_now = (int(seed) + int(seed_word)) & _MASK64
    k = (seed_now, float(p), int(ld), key)
    if k not in _masks:
        idx = (rows * ld + cols).clamp_min(0).numpy().astype(np.uint64)       # (dropped elements: any index, never stored)
        _masks[k] = torch.from_numpy(keep_mult(seed_now, idx, p))
    return _masks[k]


def epilogue_ref(P, c_prev, ldc, *, alpha=1.0, bias=None, rowbias=None, preact=None, act=ACT_NONE, dact_src=None,
                 out_drop=None, seed_word=0, residual=None, accumulate=False, c_win=None, c_bf16=False, pre_value=None,
                 dtype=torch.float64):
    """P: (M, N) product.  c_prev: the C buffer before the call, any shape with rows of ldc elements.
    bias (N); rowbias = (table, rb_ld, rb_div, rb_mod); preact / dact_src / residual = (tensor, ld) -- of preact only the
    dtype is read; out_drop = (p, seed, ld) or None, seed_word the value of the device word added to the seed;
    c_win = (nodes, Lin, Lout, stride_t, taps, Cw, pad) or None; c_bf16: C is a bf16 tensor.
    pre_value: the (M, N) pre-activation the kernel stored -- when given, the rest of the epilogue is evaluated at it
    (a bf16 pre-activation: one rounding flip must not be counted a second time in C).
    Returns (expected C buffer in c_prev's shape, expected pre-activation or None, dropout multipliers or None)."""
    M, N = P.shape
    v = float(alpha) * P.detach().cpu().to(dtype)
    if bias is not None:
        v = v + bias.detach().cpu().to(dtype)[None, :N]
    if rowbias is not None:
        table, rb_ld, rb_div, rb_mod = rowbias
        rr = (torch.arange(M) // rb_div) % rb_mod
        v = v + table.detach().cpu().reshape(-1)[: rb_mod * rb_ld].view(rb_mod, rb_ld)[:, :N].to(dtype)[rr]
    pre = None
    if preact is not None:
        pre = v.clone()
        if preact[0].dtype == torch.bfloat16:
            pre = round_bf16(v)
            v = pre
        if pre_value is not None:
            v = pre_value.detach().cpu().to(dtype)
    if dact_src is not None:
        if act == ACT_NONE:
            raise ValueError("dact_src needs act to name the activation whose derivative is taken")
        v = v * _ACT[act][1](_view2d(dact_src[0], dact_src[1], M, N, dtype))
    elif act != ACT_NONE:
        v = _ACT[act][0](v)
    rows, cols, valid = targets(M, N, c_win)
    mult = None
    if out_drop is not None and out_drop[0] > 0:
        p, seed, ld = out_drop
        mult = keep_mask(p, seed, ld, seed_word, rows, cols, (M, N, c_win))
        v = v * mult.to(dtype)
    if residual is not None:
        v = v + _view2d(residual[0], residual[1], M, N, dtype)
    out = c_prev.detach().cpu().to(dtype).clone()
    flat = out.view(-1)
    pos = (rows * ldc + cols)[valid]
    v = v[valid]
    if accumulate:
        v = v + flat[pos]
    if c_bf16:
        v = round_bf16(v)
    flat[pos] = v
    return out, pre, mult
