"""Cost of the significance feature at the full split's size: S = 2149 windows, L_out = 12, N = 2911.  Recorded, not gated.

  * metrics_window_kernel per batch of B = 16 (the model's permuted output view against the dataset's target layout), next to
    metrics_kernel (tecm_metrics_accumulate) on the same operands; algorithmic bytes: two reads of B*H*N*4 B (the table
    written is B*H*64 B);
  * block_bootstrap_kernel on a (M, S, W) = (4, 2149, 96) table, R = 1000 replicates, block length 120, G = 1 and 4;
    algorithmic bytes: every replicate reads every forecast's S rows once, R*M*S*W*8 B (from a 6.6 MB table: cache traffic),
    and writes R*M*G*W*8 B;
    kernel times: a run of its own under `rocprofv3 --kernel-trace --stats` (a child process started before this one touches
    the GPU), read from the trace database, first launch of every case dropped;
  * wall time of `evaluate_significance` (model + historical average, R = 1000) against `evaluate_split` over the same 20
    batches at B = 16 (L_in = 48, fp32), each ending in a device synchronise, median of `--passes` alternating passes after
    one warm-up pass.

    python tools/significance_bench.py [--out PREFIX] [--no-profile]        # writes PREFIX.json and PREFIX.txt
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

S = 2149
B = 16
M, R, BLOCK = 4, 1000, 120
W = L_OUT * 8
GROUPS = (1, 4)
PROFILE_LAUNCHES = 10
SCALER = (20.0, 8.0)


def batch_operands():
    import torch
    torch.manual_seed(0)
    pred = torch.randn(B, N, L_OUT, device="cuda").permute(0, 2, 1).unsqueeze(-1)       # the model's output view
    y = torch.randn(B, L_OUT, N, 1, device="cuda")
    return pred, y


def bootstrap_case(G):
    import torch
    from tecmollm.significance import bootstrap_sums, draw_starts
    gen = torch.Generator(device="cuda").manual_seed(G)
    table = torch.randn(M, S, W, device="cuda", dtype=torch.float64, generator=gen)
    starts = draw_starts(S, BLOCK, R, seed=0).cuda()
    ids = (torch.arange(S, device="cuda") % G).to(torch.int32) if G > 1 else None
    return lambda: bootstrap_sums(table, starts, BLOCK, ids, G)


def kernels_only():
    """The child run under the profiler: per case one warm-up launch and PROFILE_LAUNCHES more."""
    import torch
    from src.evaluation.metrics import HorizonMetrics
    from tecmollm.significance import window_stats
    pred, y = batch_operands()
    table = torch.zeros(S, L_OUT, 8, device="cuda", dtype=torch.float64)
    hm = HorizonMetrics(L_OUT, SCALER)
    for _ in range(1 + PROFILE_LAUNCHES):
        window_stats(pred, y, table, None, 0, SCALER)
    torch.cuda.synchronize()
    for _ in range(1 + PROFILE_LAUNCHES):
        hm.update(pred, y)
    torch.cuda.synchronize()
    for G in GROUPS:
        launch = bootstrap_case(G)
        for _ in range(1 + PROFILE_LAUNCHES):
            launch()
        torch.cuda.synchronize()


def profile_kernels(timeout=600):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "significance", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, start, end from kernels order by start").fetchall()
    per = 1 + PROFILE_LAUNCHES
    window = [(e - s) / 1e3 for name, s, e in rows if "metrics_window_kernel" in name]
    pooled = [(e - s) / 1e3 for name, s, e in rows if "metrics_kernel" in name]
    boot = [(e - s) / 1e3 for name, s, e in rows if "block_bootstrap_kernel" in name]
    if len(window) != per or len(pooled) != per or len(boot) != per * len(GROUPS):
        raise RuntimeError(f"unexpected launch counts: {len(window)} window, {len(pooled)} pooled, {len(boot)} bootstrap")
    summary = lambda u: (len(u), float(np.mean(u)), float(np.min(u)), float(np.max(u)))
    out = {"metrics_window_kernel": summary(window[1:]), "metrics_kernel": summary(pooled[1:])}
    for c, G in enumerate(GROUPS):
        out[G] = summary(boot[c * per + 1:(c + 1) * per])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "significance"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (kernel time: not measured)")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    kern = {} if a.no_profile else profile_kernels()                       # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("significance_bench.py measures on the GPU; none found")
    from tecmollm import evaluate as E
    from tecmollm import significance as SG
    dev_name = torch.cuda.get_device_name(0)
    lines, rows = [f"# {dev_name}; S = {S}, L_out = {L_OUT}, N = {N}; python tools/significance_bench.py"
                   + (" --no-profile" if a.no_profile else "") + f" --passes {a.passes}"], []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    batch = 2 * B * L_OUT * N * 4
    for name in ("metrics_window_kernel", "metrics_kernel"):
        if name in kern:
            cnt, us, lo, hi = kern[name]
            rows.append(dict(kernel=name, B=B, algorithmic_bytes=batch, kernel_us=us, kernel_us_min=lo, kernel_us_max=hi,
                             launches=cnt, algorithmic_GBps=batch / us / 1e3))
            say(f"{name}, B = {B}: {us:.1f} us (min {lo:.1f}, max {hi:.1f}; rocprofv3 kernel trace, {cnt} launches), "
                f"algorithmic {batch / 1e6:.2f} MB -> {batch / us / 1e3:.0f} GB/s")
    for G in GROUPS:
        if G in kern:
            cnt, us, lo, hi = kern[G]
            read, written = R * M * S * W * 8, R * M * G * W * 8
            rows.append(dict(kernel="block_bootstrap_kernel", G=G, R=R, M=M, S=S, W=W, block_len=BLOCK, table_bytes=M * S * W * 8,
                             read_bytes=read, written_bytes=written, kernel_us=us, kernel_us_min=lo, kernel_us_max=hi,
                             launches=cnt, read_GBps=read / us / 1e3))
            say(f"block_bootstrap_kernel, G = {G}, R = {R}, M = {M}, W = {W}, L = {BLOCK}: {us:.1f} us (min {lo:.1f}, max {hi:.1f}; "
                f"rocprofv3 kernel trace, {cnt} launches); reads {read / 1e9:.2f} GB of a {M * S * W * 8 / 1e6:.1f} MB table "
                f"-> {read / us / 1e3:.0f} GB/s, writes {written / 1e6:.1f} MB")
    if not kern:
        say("kernel time: not measured")
    # ---------------------------------------------------------------- evaluate_significance against evaluate_split
    from oracle import ref_cpu as Rf
    from src.model.tec_mollm import TEC_MoLLM
    cfg = Rf.default_config(L_in=48, L_out=L_OUT, num_nodes=N)
    torch.manual_seed(3)
    with torch.device("cuda"):
        model = TEC_MoLLM(dict(cfg, include_wte=False, load_pretrained_gpt2=False)).eval()
    X, TF = split_arrays()
    ds = dataset(X, TF, 48)
    ei = Rf.grid_graph()[0].cuda()
    order = list(range(20 * B))
    got = {}

    def split():
        got["split"] = E.evaluate_split(model, ds, ei, B, scaler=SCALER, order=order)

    def significance():
        got["sig"] = SG.evaluate_significance(model, ds, ei, B, scaler=SCALER, order=order, replicates=R)
    runs = {"evaluate_split": split, "evaluate_significance": significance}
    times = {k: [] for k in runs}
    for p in range(1 + a.passes):
        for k, fn in runs.items():
            s = wall(fn)
            if p:
                times[k].append(s)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    keys = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg")         # the pooled sums are atomic adds: equal to rounding
    gap = max(abs(got["sig"][0][n][k] - got["split"][n][k]) / abs(got["split"][n][k]) for n in got["split"] for k in keys)
    say(f"20 batches at B = {B}, L_in = 48, fp32, model + historical average: evaluate_split {med['evaluate_split']:.3f} s, "
        f"evaluate_significance (R = {R}, block length {got['sig'][1]['block_len']}, table of {len(ds)} windows) "
        f"{med['evaluate_significance']:.3f} s, ratio {med['evaluate_significance'] / med['evaluate_split']:.3f}; largest relative "
        f"difference of the two results' averages {gap:.1e}  (host clock around a synchronise, median of {a.passes} alternating passes; all passes: {times})")
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, S=S, L_out=L_OUT, N=N, kernel=rows,
                       end_to_end=dict(batches=20, B=B, L_in=48, replicates=R, median_s=med, all_s=times, results_max_rel_diff=gap)),
                  f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
