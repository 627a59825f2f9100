"""Cost of the per-cell evaluation statistics (MapMetrics / tecm_metrics_map) at the full grid: N = 2911, L_out = 12, B = 16.
Recorded, not gated.

  * kernel time of metrics_map_kernel: a run of its own under `rocprofv3 --kernel-trace --stats` (a child process started
    before this one touches the GPU), read from the trace database, first launch of every case dropped.  Cases: the model's
    permuted output against the dataset target (the LDS path) and a stride-0 baseline view against it, with 1 and 4 groups;
  * algorithmic bytes per update: two operands of S*H*I*4 B (one of S*I*4 B for the stride-0 view) plus a read and a write
    of H*I*64 B of statistics per group present;
  * wall time of evaluate_maps against evaluate_split over the same 20 batches at B = 16, L_in = 48 (the set-up of
    tools/baseline_bench.py: fp32, model + historical average), alternating, one warm-up pass each, with 1 and 4 groups.

    python tools/error_maps_bench.py [--out PREFIX] [--no-profile]           # writes PREFIX.json and PREFIX.txt
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

B = 16
PROFILE_LAUNCHES = 20
CASES = [("model output", "model", 1), ("model output", "model", 4), ("stride-0 baseline", "baseline", 1),
         ("stride-0 baseline", "baseline", 4)]


def algorithmic_bytes(kind, G):
    pred = B * N * 4 * (L_OUT if kind == "model" else 1)
    return pred + B * L_OUT * N * 4 + 2 * G * L_OUT * N * 64


def kernels_only():
    """The child run under the profiler: per case one warm-up update and PROFILE_LAUNCHES more, cases in CASES order."""
    import torch
    from src.evaluation.metrics import MapMetrics
    torch.manual_seed(0)
    y = torch.randn(B, L_OUT, N, 1, device="cuda")
    out = torch.randn(B, N, L_OUT, device="cuda").permute(0, 2, 1).unsqueeze(-1)
    base = torch.randn(B, N, device="cuda").view(B, 1, N, 1).expand(B, L_OUT, N, 1)
    for _, kind, G in CASES:
        mm = MapMetrics(L_OUT, N, G, (20.0, 8.0))
        ids = (torch.arange(B, device="cuda", dtype=torch.int32) % G) if G > 1 else None
        for _ in range(1 + PROFILE_LAUNCHES):
            mm.update(out if kind == "model" else base, y, ids)
        torch.cuda.synchronize()


def profile_kernels(timeout=420):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "maps", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, start, end from kernels order by start").fetchall()
    us = [(e - s) / 1e3 for name, s, e in rows if "metrics_map_kernel" in name]
    if len(us) != len(CASES) * (1 + PROFILE_LAUNCHES):
        raise RuntimeError(f"expected {len(CASES) * (1 + PROFILE_LAUNCHES)} launches of metrics_map_kernel, saw {len(us)}")
    out = []
    for c in range(len(CASES)):
        u = us[c * (1 + PROFILE_LAUNCHES) + 1:(c + 1) * (1 + PROFILE_LAUNCHES)]
        out.append((len(u), float(np.mean(u)), float(np.min(u)), float(np.max(u))))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error_maps"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (kernel time: not measured)")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    kern = [] if a.no_profile else profile_kernels()                       # before this process opens the GPU
    import torch
    from tecmollm import evaluate as E
    if not torch.cuda.is_available():
        raise SystemExit("error_maps_bench.py measures on the GPU; none found")
    dev_name = torch.cuda.get_device_name(0)
    lines, rows = [f"# {dev_name}; N = {N}, L_out = {L_OUT}, B = {B}"], []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    for (label, kind, G), k in zip(CASES, kern):
        cnt, us, lo, hi = k
        nbytes = algorithmic_bytes(kind, G)
        rows.append(dict(operand=label, groups=G, algorithmic_bytes=nbytes, kernel_us=us, kernel_us_min=lo, kernel_us_max=hi,
                         launches=cnt, algorithmic_GBps=nbytes / us / 1e3))
        say(f"metrics_map_kernel, {label}, {G} group(s): {us:.1f} us (min {lo:.1f}, max {hi:.1f}; rocprofv3 kernel trace, {cnt} "
            f"launches), algorithmic {nbytes / 1e6:.2f} MB -> {nbytes / us / 1e3:.0f} GB/s")
    if not kern:
        say("kernel time: not measured")
    from oracle import ref_cpu as R
    from src.model.tec_mollm import TEC_MoLLM
    cfg = R.default_config(L_in=48, L_out=L_OUT, num_nodes=N)
    torch.manual_seed(3)
    with torch.device("cuda"):
        model = TEC_MoLLM(dict(cfg, include_wte=False, load_pretrained_gpt2=False)).eval()
    X, TF = split_arrays()
    ds = dataset(X, TF, 48)
    ei = R.grid_graph()[0].cuda()
    order = list(range(20 * B))
    g4 = (torch.arange(len(ds), device="cuda", dtype=torch.int32) // 3) % 4
    runs = {"evaluate_split": lambda: E.evaluate_split(model, ds, ei, B, scaler=(20.0, 8.0), order=order),
            "evaluate_maps G=1": lambda: E.evaluate_maps(model, ds, ei, B, scaler=(20.0, 8.0), order=order),
            "evaluate_maps G=4": lambda: E.evaluate_maps(model, ds, ei, B, scaler=(20.0, 8.0), order=order, groups=g4,
                                                         num_groups=4)}
    times = {k: [] for k in runs}
    for p in range(1 + a.passes):
        for k, fn in runs.items():
            s = wall(fn)
            if p:
                times[k].append(s)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    say("20 batches at B = 16, L_in = 48, fp32, model + historical average, median wall of "
        f"{a.passes} alternating passes: " + ", ".join(f"{k} {v:.3f} s" for k, v in med.items())
        + f"; ratios to evaluate_split {med['evaluate_maps G=1'] / med['evaluate_split']:.3f} and "
        f"{med['evaluate_maps G=4'] / med['evaluate_split']:.3f}  (all passes: {times})")
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, kernel=rows, maps_vs_split=dict(batches=20, B=B, L_in=48, median_s=med, all_s=times)),
                  f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
