#!/usr/bin/env python3
"""Timing of the long-window attention kernels (csrc/attention_long.hip, 33 <= T <= 1024) and of a training step that uses
them (diagnostics, not the bench).

    python tools/attention_long_bench.py                       # every instance, B = 2, N = 2911, T in {33, 45, 64, 128}
    python tools/attention_long_bench.py --step                # + one TrainStep at L_in = 720 (T = 45), B = 2, fp32 and bf16
    python tools/attention_long_bench.py --step-only --precision bf16 --steps 3   # the step alone (for a rocprofv3 run)

The HBM bound of a launch is its algorithmic bytes (qkv read, ctx written; backward: qkv and dctx read, dqkv written, each
once) over 6.29 TB/s, the measured float4 copy rate of an MI355X; `frac` = that bound / the measured time.  TFLOP/s counts the
algorithmic causal work per (sequence, head), 128*T*(T+1) forward and 448*T*(T+1) backward (the kernel itself recomputes
P and dP in each of its three passes: 576*T*(T+1)).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM = 6.29e12
H, D = 12, 768


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us


def _row(pass_, T, qkv, dctx, out, us, by, fl):
    return dict(pass_=pass_, T=T, qkv=qkv, dctx=dctx, out=out, us=round(us, 1), GB=round(by / 1e9, 3),
                bound_us=round(by / HBM * 1e6, 1), frac=round(by / HBM * 1e6 / us, 3), TFLOPs=round(fl / us / 1e6, 1))


def kernels(B, N, lengths, reps, p):
    from tecmollm import ops
    dev = torch.device("cuda")
    drop = ops.drop(p, 1234, 1) if p else None
    rows = []
    for T in lengths:
        g = torch.Generator(device=dev).manual_seed(T)
        qkv32 = torch.randn(B, T, N, 3 * D, device=dev, generator=g) * 0.5
        dctx32 = torch.randn(B, T, N, D, device=dev, generator=g)
        tokens = B * T * N
        name = {False: "f32", True: "bf16"}
        for q16 in (False, True):
            qkv = qkv32.bfloat16() if q16 else qkv32
            for o16 in (False, True):
                ctx = torch.empty(B, T, N, D, device=dev, dtype=torch.bfloat16 if o16 else torch.float32)
                us = _time(lambda: ops.attention_fwd(qkv, ctx, B, T, N, H, D, drop), reps)
                by = tokens * (3 * D * qkv.element_size() + D * ctx.element_size())
                rows.append(_row("fwd", T, name[q16], "-", name[o16], us, by, 128.0 * T * (T + 1) * B * N * H))
        for q16, d16 in ((False, False), (True, False), (True, True)):
            qkv = qkv32.bfloat16() if q16 else qkv32
            dctx = dctx32.bfloat16() if d16 else dctx32
            for o16 in (False, True):
                dq = torch.empty(B, T, N, 3 * D, device=dev, dtype=torch.bfloat16 if o16 else torch.float32)
                us = _time(lambda: ops.attention_bwd(qkv, dctx, dq, B, T, N, H, D, drop), reps)
                by = tokens * (3 * D * qkv.element_size() + D * dctx.element_size() + 3 * D * dq.element_size())
                rows.append(_row("bwd", T, name[q16], name[d16], name[o16], us, by, 448.0 * T * (T + 1) * B * N * H))
        del qkv32, dctx32, qkv, dctx
        torch.cuda.empty_cache()
    return rows


def train_step(precision, L_in, B, steps, warmup):
    """ms per TrainStep (training mode, dropout on) at the bench's model configuration (N = 2911, F = 10), L_in / B given."""
    from oracle import ref_cpu as R
    from src.model.tec_mollm import TEC_MoLLM
    from tecmollm.synthetic import grid_graph, synthetic_batch
    from tecmollm.train import TrainStep
    dev = torch.device("cuda")
    cfg = R.default_config(L_in=L_in, L_out=12, num_nodes=2911, c_in=10, d_emb=12)
    mc = dict(cfg, gat_graphs="per_timestep", include_wte=False, load_pretrained_gpt2=False, precision=precision)
    torch.manual_seed(0)
    model = TEC_MoLLM(mc).to(dev).train()
    ei, ew = grid_graph()
    ei, ew = ei.to(dev), ew.to(dev)
    x, tf, y = synthetic_batch(B, L_in, 2911, 10, 12, seed=1234)
    x, y = x.to(dev), y.to(dev)
    tf = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(B, L_in, 2911, 4)
    ts = TrainStep(model, world_size=1)
    for _ in range(warmup):
        ts.step(x, tf, ei, ew, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ts.step(x, tf, ei, ew, y)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    T = (L_in // 4) // cfg["patch_len"]
    del ts, model
    torch.cuda.empty_cache()
    return dict(precision=precision, L_in=L_in, T=T, B=B, steps=steps, ms_per_step=round(ms, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=2)
    ap.add_argument("--N", type=int, default=2911)
    ap.add_argument("--T", type=int, nargs="*", default=[33, 45, 64, 128])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--p", type=float, default=0.1, help="attention dropout (the training step's)")
    ap.add_argument("--step", action="store_true", help="also time one TrainStep at --L_in, in each --precision")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--precision", choices=["fp32", "bf16"], nargs="*", default=["fp32", "bf16"])
    ap.add_argument("--L_in", type=int, default=720)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None, help="write every row here as well")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {}
    if not a.step_only:
        rows = kernels(a.B, a.N, a.T, a.reps, a.p)
        print(f"attention, B = {a.B}, N = {a.N}, H = {H}, dropout p = {a.p}; bound = bytes / {HBM / 1e12:.2f} TB/s")
        print(f"{'pass':4s} {'T':>4s} {'qkv':>4s} {'dctx':>4s} {'out':>4s} {'us':>9s} {'GB':>7s} {'bound us':>9s} {'frac':>6s} "
              f"{'TFLOP/s':>8s}")
        for r in rows:
            print(f"{r['pass_']:4s} {r['T']:4d} {r['qkv']:>4s} {r['dctx']:>4s} {r['out']:>4s} {r['us']:9.1f} {r['GB']:7.3f} "
                  f"{r['bound_us']:9.1f} {r['frac']:6.3f} {r['TFLOPs']:8.1f}", flush=True)
        out["kernels"] = rows
    if a.step or a.step_only:
        out["steps"] = []
        for prec in a.precision:
            r = train_step(prec, a.L_in, a.B, a.steps, a.warmup)
            print("train step:", json.dumps(r), flush=True)
            out["steps"].append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
