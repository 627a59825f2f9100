"""Activation memory of one TEC_MoLLM step, and the recompute level the step runs at (functions.DropPlan.recompute).

Level 0 keeps every activation a backward reads (the launch sequence the project always had).  Level 1: each GPT-2 block
keeps its input h only and re-runs its forward just before its backward (GPT2StackFn).  Level 2: level 1, and each conv
block keeps what it received and rebuilds y, the GroupNorm statistics and act in its backward (ConvBlockFn).  The rebuilt
tensors are the forward's bit for bit: the same kernels, the same arguments, the same dropout plan.

`estimate` replays the allocations the autograd Functions make -- tensor by tensor, in their order, with the points where
each is dropped -- for one step: the forward, and with grad on the backward with its gradient hand-over (TrainStep: the
gradients autograd returns stay alive until the flat buffer absorbs them).  Tensors below about a megabyte (statistics,
bias vectors, packed conv weights, reduction scratch) are left out.  `choose` takes the smallest level whose estimate fits.
"""
from __future__ import annotations

import logging
import os
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

import torch

log = logging.getLogger(__name__)

ENV = "TECM_RECOMPUTE"        # diagnostics: "0" / "1" / "2" force a level, "budget:<GB>" replaces the device's free memory
MARGIN_MIN = 1 << 30          # the budget keeps max(1 GiB, 5 % of the device) free: allocator rounding, the tensors left
MARGIN_FRAC = 0.05            # out here, other streams' work
LEVELS = (0, 1, 2)

D_LLM, LORA_R, F3, F4 = 768, 32, 2304, 3072


@dataclass(frozen=True)
class Estimate:
    kept: int          # bytes live at the end of the forward: what the backward reads, and the output
    transient: int     # the step's largest working set on top of `kept` (forward or backward)

    @property
    def peak(self) -> int:
        return self.kept + self.transient


class _Sim:
    """Live bytes of a sequence of allocations and releases (sizes rounded as the caching allocator rounds them)."""

    def __init__(self):
        self.live: Dict[str, int] = {}
        self.cur = 0
        self.peak = 0

    def new(self, name: str, nbytes: int) -> None:
        n = 0 if nbytes <= 0 else (int(nbytes) + 511) // 512 * 512
        self.cur += n                                        # a rebound name: the new tensor exists before the old one goes
        self.peak = max(self.peak, self.cur)
        self.drop(name)
        self.live[name] = n

    def drop(self, *names: str) -> None:
        for nm in names:
            self.cur -= self.live.pop(nm, 0)

    def drop_prefix(self, prefix: str) -> None:
        self.drop(*[k for k in self.live if k.startswith(prefix)])


def _gpt_flags(prec: int):
    from . import functions as F_
    b16 = prec == 1
    return b16, b16 and F_.QKV16, b16 and F_.PRE16, b16 and F_.GRAD16


def _block_fwd(s: _Sim, tag: str, M: int, prec: int, training: bool, keep: bool, out: bool) -> None:
    """functions.GPT2StackFn._block_fwd: names `tag`.<tensor>; with keep the acts stay live, h3 is `tag`.h3."""
    b16, q16, p16, _ = _gpt_flags(prec)
    KE, D = D_LLM + LORA_R, D_LLM
    s.new(tag + ".st1", M * 8)
    s.new(tag + ".u", M * KE * (2 if b16 else 4))
    if b16 and training:
        s.new(tag + ".ud", M * D * 2)
        if not keep:
            s.drop(tag + ".ud")
    s.new(tag + ".qkv", M * F3 * (2 if q16 else 4))
    if not keep:
        s.drop(tag + ".u")
    s.new(tag + ".cx", M * D * (2 if b16 else 4))
    if not keep:
        s.drop(tag + ".qkv")
    s.new(tag + ".h2", M * D * 4)
    if not keep:
        s.drop(tag + ".cx")
    s.new(tag + ".st2", M * 8)
    s.new(tag + ".u2", M * D * (2 if b16 else 4))
    s.new(tag + ".a", M * F4 * (2 if p16 else 4))
    s.new(tag + ".f", M * F4 * (2 if b16 else 4))
    if not keep:
        s.drop(tag + ".u2", tag + ".a")
    if out:
        s.new(tag + ".h3", M * D * 4)
    s.drop(tag + ".cx", tag + ".u2", tag + ".f")
    if not keep:
        s.drop(tag + ".h2", tag + ".st1", tag + ".st2")


def layer_bytes_per_token(prec: int, training: bool) -> int:
    """Bytes a GPT-2 block keeps for its backward per token at level 0: its input h and what _block_fwd returns."""
    s = _Sim()
    M = 1 << 20
    _block_fwd(s, "x", M, int(prec), training, keep=True, out=False)
    return (s.cur + 4 * D_LLM * M) // M


def conv_bytes_per_step(cfg: dict, prec: int) -> float:
    """Bytes both conv blocks keep for their backward at level 0 per (input time step, node) of one sample: each block's
    input (and its bf16 copy where kept), y and act; the statistics are left out."""
    N = 1 << 10
    L = int(cfg["temporal_seq_len"])
    tot = 0
    in16 = int(prec) == 1
    for b in _conv_dims(cfg, 1, N, int(prec)):
        inp = b["Lc"] * N * b["ld_in"]
        tot += 4 * inp + (2 * inp if (in16 and b["r16"]) else 0) + b["y"] + b["act"]
        in16 = b["r16"]
    return tot / (L * N)


def _stack_fwd(s: _Sim, M: int, S: int, n_layers: int, prec: int, training: bool, level: int, keep: bool,
               fused: bool, h0: str) -> None:
    """GPT2StackFn.forward on the tensor `h0`: leaves `stack.out` live, and what the backward reads as `stack.keep*`."""
    h = h0
    for i in range(n_layers):
        tag = f"L{i}"
        _block_fwd(s, tag, M, prec, training, keep=keep and level == 0, out=True)
        if keep and level == 0:
            for t in ("st1", "u", "ud", "qkv", "h2", "st2", "a"):
                if tag + "." + t in s.live:
                    s.live["stack.keep." + tag + "." + t] = s.live.pop(tag + "." + t)
        nxt = f"stack.h{i + 1}"
        s.live[nxt] = s.live.pop(tag + ".h3")
        if not keep and h != h0:
            s.drop(h)                                        # the lean forward: the previous block's output is gone
        h = nxt
    s.new("stack.out", M * D_LLM * (2 if fused else 4))
    if not keep:
        s.drop(h)


def _stack_bwd(s: _Sim, M: int, n_layers: int, prec: int, training: bool, level: int, dout: str) -> None:
    """GPT2StackFn.backward: consumes `dout`, leaves `stack.dh`; releases what the forward kept."""
    b16, q16, _, g16 = _gpt_flags(prec)
    D, KE = D_LLM, D_LLM + LORA_R
    mb = (2 if b16 else 4) * M * D                            # masked_buf: bf16 when the GEMM behind it reads a bf16 weight
    s.new("bw.dh", 4 * M * D)
    if training:
        s.new("bw.dhm", mb)
    for i in reversed(range(n_layers)):
        tag = f"R{i}"
        if level:
            _block_fwd(s, tag, M, prec, training, keep=True, out=False)
        s.new("bw.da", M * F4 * (2 if b16 else 4))
        s.new("bw.du2", M * D * (2 if g16 else 4))
        s.drop("bw.da")
        s.new("bw.dh2", 4 * M * D)
        if training:
            s.new("bw.dh2m", mb)
        c16 = g16 and q16 and training
        if c16:
            s.new("bw.dcx", 2 * M * D)
        elif g16:
            s.new("bw.dcx", 4 * M * D)
        s.new("bw.dqkv", M * F3 * (2 if b16 else 4))
        s.new("bw.du", M * KE * (2 if (g16 and b16) else 4))
        s.new("bw.dzA", M * D * (2 if g16 else 4))
        s.new("bw.dhn", 4 * M * D)
        if training and i > 0:
            s.new("bw.dhm_next", mb)
        s.drop("bw.dhm")
        if "bw.dhm_next" in s.live:
            s.live["bw.dhm"] = s.live.pop("bw.dhm_next")
        s.drop("bw.dh")
        s.live["bw.dh"] = s.live.pop("bw.dhn")
        if level:
            s.drop_prefix(tag + ".")
            s.drop("bw.du2", "bw.dh2", "bw.dh2m", "bw.dcx", "bw.dqkv", "bw.du", "bw.dzA")
        # (level 0 with the batched gamma / beta reduction drops dzA here as well and keeps the (blocks, 2D) partials of every
        #  LayerNorm -- 6 MB each -- to the end instead: the estimate counts neither and stays an upper bound by 4 M D bytes)
    s.drop_prefix("stack.keep.")
    s.drop_prefix("stack.h")
    s.drop("bw.du2", "bw.dh2", "bw.dh2m", "bw.dcx", "bw.dqkv", "bw.du", "bw.dzA", "bw.dhm", dout)
    s.live["stack.dh"] = s.live.pop("bw.dh")


def _conv_dims(cfg: dict, B: int, N: int, prec: int):
    """Per conv block: its lengths and the bytes of what ConvBlockFn allocates, with the storage policy it applies."""
    from . import functions as F_
    from . import ops
    L = int(cfg["temporal_seq_len"])
    blocks = []
    ld_in, Lc = F_.CP, L
    in16 = prec == 1 and ld_in % 8 == 0 and os.environ.get("TECM_XS16", "1")[:1] != "0"
    for Cout, st in zip(cfg["temporal_channel_list"], cfg["temporal_strides"]):
        CT = 3 * Cout
        Lo = (Lc - 1) // st + 1
        r16 = prec == 1 and F_.conv_block_acts16(Lc, N, Cout)
        seq16 = r16 and in16
        seq_f32 = (not seq16) and prec == 0
        fwd_seq = (seq16 or seq_f32) and ops.conv_fwd_seq_ok(Lc, Cout, ld_in, f32=seq_f32)
        y16 = r16 and fwd_seq and seq16 and F_.conv_block_y16(Lc, N, Cout, ld_in)
        compact = st > 1 and ops.gn_reg_ok(Lc, N, Cout) and prec in (0, 1)
        La = Lo if compact else Lc
        adt = 2 if r16 else 4
        twin = r16 and compact and Cout % 8 == 0 and ops.tn_ok(Cout, CT, B * Lo * N)
        d16 = r16 and ops.uses_bf16(CT, Cout, Cout, CT, b_layout=ops.B_KN)
        blocks.append(dict(Lc=Lc, Lo=Lo, Cout=Cout, ld_in=ld_in, y=B * Lc * N * CT * (2 if y16 else 4),
                           act=B * La * N * CT * adt, out=B * Lo * N * Cout * 4, out16=B * Lo * N * Cout * 2 if r16 else 0,
                           r16=r16, twin=B * Lo * N * Cout * 2 if twin else 0,
                           dact=B * Lo * N * CT * (2 if d16 else 4), dy=B * Lc * N * CT * adt,
                           dinp=B * Lc * N * ld_in * 4))
        in16 = r16
        ld_in, Lc = Cout, Lo
    return blocks


def _head_dims(cfg: dict, B: int, N: int, T: int):
    K1 = T * D_LLM
    Hd = K1 // 4
    return B * N, K1, Hd, int(cfg["prediction_horizon"])


def _trainable_bytes(cfg: dict, T: int, N: int) -> int:
    """fp32 bytes of every trainable parameter (= the gradients one backward hands over)."""
    S, K1, Hd, Lo = _head_dims(cfg, 1, N, T)
    n = Hd * K1 + Hd + Lo * Hd + Lo                                           # head
    C2 = cfg["temporal_channel_list"][-1]
    n += D_LLM * cfg["patch_len"] * C2 + D_LLM + 1024 * D_LLM                # patch projection, wpe
    n += cfg["llm_layers"] * (LORA_R * D_LLM + F3 * LORA_R + 4 * D_LLM) + 2 * D_LLM
    cin, C = cfg["spatial_in_channels_base"], cfg["spatial_in_channels_base"] + cfg["d_emb"]
    for Cout in cfg["temporal_channel_list"]:
        n += 15 * Cout * cin + 9 * Cout + Cout * 3 * Cout + Cout
        cin = Cout
    n += (N + 12 + 366 + cfg.get("num_years", 13) + 4) * cfg["d_emb"] + 2 * C * C + 4 * C
    return 4 * n


def estimate(cfg: dict, B: int, prec: int, level: int, training: bool, grad: bool, fuse_head: bool = True,
             embd_masked_grad: bool = True) -> Estimate:
    """Bytes one TEC_MoLLM step allocates on top of what exists before it (parameters, optimizer state, cached weight
    copies).  cfg: the model_config dict; prec: ops.PREC_*; training: model.training (dropout on); grad: a backward follows
    (False: the lean forward of functions.DropPlan.keep = False, whatever the level).  fuse_head / embd_masked_grad: the
    DropPlan fields of the same names as TEC_MoLLM.forward sets them (bf16 and fp32 mode / every mode but bf16)."""
    from . import functions as F_
    prec = int(prec)
    N = int(cfg["num_nodes"])
    L = int(cfg["temporal_seq_len"])
    blocks = _conv_dims(cfg, B, N, prec)
    T = blocks[-1]["Lo"] // int(cfg["patch_len"])
    M = B * T * N
    S, K1, Hd, Lout = _head_dims(cfg, B, N, T)
    keep = bool(grad)
    lv = level if keep else 0
    fused16 = fuse_head and prec == 1                   # ln_f writes the head's operand: bf16 ...
    fused = fused16 or (fuse_head and prec == 0)        # ... or fp32 (same bytes as ln_f's plain output, no dropped copy)
    s = _Sim()
    # ---- forward
    s.new("xs", B * L * N * F_.CP * 4)                                        # SpatialFn output
    if prec == 1 and os.environ.get("TECM_XS16", "1")[:1] != "0":
        s.new("xs16", B * L * N * F_.CP * 2)
    cur, cur16 = "xs", ("xs16" if "xs16" in s.live else None)
    for j, b in enumerate(blocks):
        s.new(f"c{j}.y", b["y"])
        s.new(f"c{j}.act", b["act"])
        s.new(f"c{j}.out", b["out"])
        if b["out16"]:
            s.new(f"c{j}.out16", b["out16"])
        if not keep or lv >= 2:
            s.drop(f"c{j}.y", f"c{j}.act")
        if cur16 is not None and not (keep and b["r16"]):
            s.drop(cur16)                                                     # the bf16 input copy: kept by bf16 blocks only
        if j > 0 and not keep:
            s.drop(cur)                                                       # the lean forward: the block's input is gone
        cur, cur16 = f"c{j}.out", (f"c{j}.out16" if b["out16"] else None)
    s.new("h0", M * D_LLM * 4)                                                # PatchEmbedFn
    if not keep or cur16 is not None:
        s.drop(cur)                                                           # the projection keeps the bf16 copy, if any
    if not keep and cur16 is not None:
        s.drop(cur16)
    _stack_fwd(s, M, S, int(cfg["llm_layers"]), prec, training, lv, keep, fused16, "h0")
    # head
    if fused16:
        s.new("hd.w1_16", Hd * K1 * 2)
        s.new("hd.w1t16", Hd * K1 * 2)
    elif training and not fused:
        s.new("hd.hd", M * D_LLM * (2 if prec == 1 else 4))
    s.new("hd.pre", S * Hd * 4)
    s.new("hd.h1", S * Hd * 4)
    s.drop("hd.w1_16")
    if not keep:
        s.drop("hd.pre", "hd.h1", "hd.hd", "hd.w1t16")
        return Estimate(kept=s.cur, transient=s.peak - s.cur)
    if training and not fused:
        s.drop("stack.out")                                                   # only the dropped copy is kept
    kept = s.cur
    # ---- backward (TrainStep: the returned gradients stay alive until the flat buffer absorbs them)
    s.new("grads", _trainable_bytes(cfg, T, N))
    s.new("hb.dpre", S * Hd * 4)
    if fused16 or (prec == 1 and training):                                   # the bf16 twin of dpre, and W1^T in bf16
        s.new("hb.dp", S * Hd * 2)
    if prec == 1 and training and not fused:
        s.new("hb.w1t16", Hd * K1 * 2)
    s.new("hb.dhid", M * D_LLM * (2 if fused16 else 4))
    s.drop("hb.dpre", "hb.dp", "hb.w1t16", "hd.pre", "hd.h1", "hd.hd", "hd.w1t16", "stack.out")
    _stack_bwd(s, M, int(cfg["llm_layers"]), prec, training, lv, "hb.dhid")
    # patch projection
    if prec == 1:
        s.new("pb.dh16", M * D_LLM * 2)
    elif training and not embd_masked_grad:                                   # else the stack's gradient arrives masked
        s.new("pb.dhm", M * D_LLM * 4)
    last = blocks[-1]
    s.new("pb.dconv", last["out"])
    s.drop("pb.dh16", "pb.dhm", "stack.dh", "h0", cur, cur16 or "")
    dcur = "pb.dconv"
    for j in reversed(range(len(blocks))):
        b = blocks[j]
        if lv >= 2:
            s.new(f"c{j}.y", b["y"])
            s.new(f"c{j}.act", b["act"])
        if b["twin"]:
            s.new("cb.twin", b["twin"])
        s.new("cb.dact", b["dact"])
        s.new("cb.dy", b["dy"])
        s.new(f"cb.dinp{j}", b["dinp"])
        s.drop("cb.twin", "cb.dact", "cb.dy", f"c{j}.y", f"c{j}.act", dcur)
        s.drop(f"c{j - 1}.out" if j > 0 else "xs", f"c{j - 1}.out16" if j > 0 else "xs16")
        dcur = f"cb.dinp{j}"
    return Estimate(kept=kept, transient=s.peak - kept)


def estimate_stack(B: int, T: int, N: int, n_layers: int, prec: int, level: int, training: bool,
                   grad: bool) -> Estimate:
    """The GPT-2 stack on its own (LLMBackbone.forward): h0 (B, T, N, 768) in, ln_f's output out."""
    M = B * T * N
    s = _Sim()
    s.new("h0", M * D_LLM * 4)
    base = s.cur
    keep = bool(grad)
    lv = level if keep else 0
    _stack_fwd(s, M, B * N, n_layers, int(prec), training, lv, keep, False, "h0")
    kept = s.cur
    if keep:
        s.new("dout", M * D_LLM * 4)
        _stack_bwd(s, M, n_layers, int(prec), training, lv, "dout")
    return Estimate(kept=kept - base, transient=s.peak - kept)


# ------------------------------------------------------------------------------------------------ policy
_CHOICES: Dict[tuple, int] = {}


def env_setting() -> Tuple[Optional[int], Optional[int]]:
    """(forced level or None, forced budget in bytes or None) from TECM_RECOMPUTE."""
    v = os.environ.get(ENV, "").strip().lower()
    if v in ("", "auto"):
        return None, None
    if v in ("0", "1", "2"):
        return int(v), None
    if v.startswith("budget:"):
        return None, int(float(v[7:]) * 1e9)
    raise ValueError(f"{ENV}={v!r}: expected 0, 1, 2, auto or budget:<GB>")


def margin(total: int) -> int:
    return max(MARGIN_MIN, int(MARGIN_FRAC * total))


def device_budget(device) -> int:
    """Bytes a step can still allocate: the device's free memory, plus what torch has reserved and not handed out, minus
    the margin."""
    free, total = torch.cuda.mem_get_info(device)
    reserved = torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
    return free + reserved - margin(total)


def pick(estimates: Callable[[int], Estimate], budget: int, levels=LEVELS) -> int:
    """The smallest level whose estimated peak fits the budget (the last one if none does)."""
    for lv in levels:
        if estimates(lv).peak <= budget:
            return lv
    return levels[-1]


def choose(key: tuple, estimates: Callable[[int], Estimate], device, levels=LEVELS, what: str = "step") -> int:
    """The level of one forward: forced by TECM_RECOMPUTE, else cached per key (shapes, precision mode, training, grad
    mode) so that it does not flip from step to step."""
    forced, budget = env_setting()
    if forced is not None:
        return min(forced, levels[-1])
    key = key + (budget,)
    lv = _CHOICES.get(key)
    if lv is None:
        b = budget if budget is not None else device_budget(device)
        lv = pick(estimates, b, levels)
        _CHOICES[key] = lv
        if lv > 0:
            e0, e = estimates(0), estimates(lv)
            log.info("%s: recompute level %d (level 0 would need %.1f GB, level %d %.1f GB, budget %.1f GB)", what, lv,
                     e0.peak / 1e9, lv, e.peak / 1e9, b / 1e9)
    return lv


def clear_choices() -> None:
    _CHOICES.clear()
