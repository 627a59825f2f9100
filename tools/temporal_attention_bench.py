"""Cost of the temporal attention export and statistics (tecm_temporal_attention, csrc/attention_probs.hip) at the full grid,
N = 2911, per GPT-2 block: (B, T) = (16, 3), (16, 6), (8, 21), (2, 90), fp32 and bf16 qkv, statistics only and statistics with
the raw export.  Recorded, not gated: nobody has measured any of this before.

  * kernel time of the new launches (att_probs_short_kernel / att_probs_long_kernel, att_probs_accumulate_kernel) and, as the
    yardstick, of the production forward kernel on the same qkv (attention_fwd_kernel* / att_long_fwd_kernel), all from ONE
    `rocprofv3 --kernel-trace --stats` run of their own (a child process started before this one touches the GPU), read from the
    trace database, first call of every case dropped; a call walks chunks of windows, so a launch's time is summed over the
    chunks of one call;
  * algorithmic bytes per call from the shapes: the q and k columns read (2/3 of qkv) plus what the launch writes (the
    workspace values and partial sums, the export), for the accumulation what it reads back plus the statistics read and
    written once; from those the share of the 8 TB/s HBM bound;
  * wall time of evaluate_temporal_attention against evaluate_split over the same 20 batches (the set-up of
    tools/baseline_bench.py: model + historical average), alternating passes, one warm-up each, compute() included.

    python tools/temporal_attention_bench.py [--out PREFIX] [--no-profile]     # writes PREFIX.json and PREFIX.txt
"""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tec-mollm_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

from baseline_bench import L_OUT, N, dataset, split_arrays, wall  # noqa: E402

HEADS, D = 12, 768
HBM_BYTES_PER_S = 8e12
REPEATS = 4
SHAPES = [(16, 3), (16, 6), (8, 21), (2, 90)]
CASES = [(B, T, dt, export) for B, T in SHAPES for dt in ("fp32", "bf16") for export in (False, True)]
PROBS = ("att_probs_short_kernel", "att_probs_long_kernel")
ACC = "att_probs_accumulate_kernel"
PROD = ("attention_fwd_kernel", "att_long_fwd_kernel")


def chunks_of(B, T):
    from tecmollm import ops
    one = ops.temporal_attention_ws_floats(1, T, N, HEADS, D, True, T <= 32)
    windows = ops.temporal_attention_ws_floats(B, T, N, HEADS, D, True, T <= 32) // one      # per chunk
    return (B + windows - 1) // windows


def algorithmic_bytes(B, T, dt, export):
    el = 4 if dt == "fp32" else 2
    ipb = 16 if T <= 32 else 4
    nb = (N + ipb - 1) // ipb
    qk = B * T * N * 2 * D * el
    ws = B * (4 * N * HEADS + nb * HEADS * T * (T + 1 if T <= 32 else 1)) * 8
    stats = (4 * N * HEADS + HEADS * T * (T + 1 if T <= 32 else 1)) * 8
    return {"probs": qk + ws + (B * N * HEADS * T * T * 4 if export else 0), "accumulate": ws + 2 * stats,
            "production": B * T * N * 3 * D * el + B * T * N * D * 4}


def kernels_only():
    """The child run under the profiler: per case one warm-up and REPEATS more of [production forward, temporal_attention]."""
    import torch
    from tecmollm import ops
    for B, T, dt, export in CASES:
        qkv = torch.randn(B * T * N, 3 * D, device="cuda").to(torch.float32 if dt == "fp32" else torch.bfloat16)
        ctx = torch.empty(B * T * N, D, device="cuda")
        st = dict(node_stats=torch.zeros(1, 1, 4, N, HEADS, device="cuda", dtype=torch.float64),
                  lag_stats=torch.zeros(1, 1, HEADS, T, device="cuda", dtype=torch.float64),
                  matrix_stats=torch.zeros(1, 1, HEADS, T, T, device="cuda", dtype=torch.float64) if T <= 32 else None,
                  counts=torch.zeros(1, device="cuda", dtype=torch.int64))
        probs = torch.empty(B, N, HEADS, T, T, device="cuda") if export else None
        for _ in range(1 + REPEATS):
            ops.attention_fwd(qkv, ctx, B, T, N, HEADS, D)
            ops.temporal_attention(qkv, B, T, N, HEADS, D, probs=probs, count=True, **st)
        torch.cuda.synchronize()
        del qkv, ctx, st, probs


def profile_kernels(timeout=540):
    """[{probs, accumulate, production: (mean us per call, min, max), chunks} per case] from a rocprofv3 run of
    `--kernels-only`."""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "tatt", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, start, end from kernels order by start").fetchall()
    mine = [(name, (e - s) / 1e3) for name, s, e in rows if any(k in name for k in PROBS + PROD + (ACC,))]
    out, at = [], 0
    for B, T, dt, export in CASES:
        chunks = chunks_of(B, T)
        per = {"probs": [], "accumulate": [], "production": []}
        for _ in range(1 + REPEATS):
            name, us = mine[at]
            if not any(k in name for k in PROD):
                raise RuntimeError(f"case {(B, T, dt, export)}: expected the production kernel, found {name}")
            per["production"].append(us)
            at += 1
            p = a_ = 0.0
            for _c in range(chunks):
                (n1, u1), (n2, u2) = mine[at], mine[at + 1]
                if not any(k in n1 for k in PROBS) or ACC not in n2:
                    raise RuntimeError(f"case {(B, T, dt, export)}: expected probs + accumulate, found {n1}, {n2}")
                p, a_, at = p + u1, a_ + u2, at + 2
            per["probs"].append(p)
            per["accumulate"].append(a_)
        res = {k: (float(np.mean(v[1:])), float(np.min(v[1:])), float(np.max(v[1:]))) for k, v in per.items()}
        res["chunks"] = chunks
        out.append(res)
    if at != len(mine):
        raise RuntimeError(f"{len(mine) - at} launches left over in the trace")
    return out


def _model():
    import torch
    from oracle import ref_cpu as R
    from src.model.tec_mollm import TEC_MoLLM
    cfg = R.default_config(L_in=48, L_out=L_OUT, num_nodes=N)
    torch.manual_seed(3)
    with torch.device("cuda"):
        return TEC_MoLLM(dict(cfg, include_wte=False, load_pretrained_gpt2=False)).eval()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_attention"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (kernel time: not measured)")
    ap.add_argument("--no-wall", action="store_true", help="skip the evaluate_temporal_attention / evaluate_split comparison")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    kern = [] if a.no_profile else profile_kernels()                       # before this process opens the GPU
    import torch
    from oracle import ref_cpu as R
    from tecmollm import evaluate as E
    from tecmollm import evaluate_temporal_attention
    if not torch.cuda.is_available():
        raise SystemExit("temporal_attention_bench.py measures on the GPU; none found")
    dev_name = torch.cuda.get_device_name(0)
    lines, rows = [f"# {dev_name}; N = {N}, 12 heads, one GPT-2 block; us per call: mean (min, max) of {REPEATS} calls, rocprofv3 "
                   "kernel trace; bytes: algorithmic"], []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    for (B, T, dt, export), per in zip(CASES, kern):
        nbytes = algorithmic_bytes(B, T, dt, export)
        row = dict(B=B, T=T, qkv=dt, export=export, chunks=per["chunks"])
        parts = []
        for k in ("probs", "accumulate", "production"):
            us, lo, hi = per[k]
            share = nbytes[k] / (us * 1e-6) / HBM_BYTES_PER_S
            row[k] = dict(us=us, us_min=lo, us_max=hi, algorithmic_bytes=nbytes[k], share_of_hbm_bound=share)
            parts.append(f"{k} {us:.1f} us ({lo:.1f}, {hi:.1f}), {nbytes[k] / 1e6:.1f} MB = {share:.3f} of the HBM bound")
        row["probs_over_production"] = per["probs"][0] / per["production"][0]
        rows.append(row)
        say(f"B={B} T={T} {dt} {'statistics + export' if export else 'statistics'} ({per['chunks']} chunk(s)): " + "; ".join(parts)
            + f"; probs / production = {row['probs_over_production']:.2f}")
    if not kern:
        say("kernel time: not measured")
    wall_res = None
    if not a.no_wall:
        B = 16
        model = _model()
        ei = R.grid_graph()[0].cuda()
        X, TF = split_arrays()
        ds = dataset(X, TF, 48)
        order = list(range(20 * B))
        runs = {"evaluate_split": lambda: E.evaluate_split(model, ds, ei, B, scaler=(20.0, 8.0), order=order),
                "evaluate_temporal_attention": lambda: evaluate_temporal_attention(model, ds, ei, B, order=order)}
        times = {k: [] for k in runs}
        for p in range(1 + a.passes):
            for k, fn in runs.items():
                s = wall(fn)
                if p:
                    times[k].append(s)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        ratio = med["evaluate_temporal_attention"] / med["evaluate_split"]
        say(f"20 batches at B = {B}, L_in = 48 (T = 3), fp32, 3 blocks, median wall of {a.passes} alternating passes: "
            + ", ".join(f"{k} {v:.3f} s" for k, v in med.items()) + f"; ratio {ratio:.3f} (both run the model's forward; "
            f"evaluate_temporal_attention's wall includes compute(); all passes: {times})")
        wall_res = dict(batches=20, B=B, L_in=48, median_s=med, all_s=times, ratio=ratio)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, kernel=rows, temporal_attention_vs_split=wall_res), f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
