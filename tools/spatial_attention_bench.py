"""Cost of the spatial attention statistics (AttentionStats / tecm_spatial_attention) at the full grid: N = 2911, L_in = 48,
B = 16, fp32, every timestep a graph (768 graphs per update).  Recorded, not gated.

  * kernel time of the three launches (spatial_attn_rows_kernel, spatial_attn_target_kernel, spatial_attn_accumulate_kernel): a
    run of its own under `rocprofv3 --kernel-trace --stats` (a child process started before this one touches the GPU), read
    from the trace database, first update of every case dropped; an update walks several chunks of graphs, so the time of a
    launch is summed over the chunks of one update.  Cases: 1 group and 12 groups (time-of-day slot of each timestep);
  * algorithmic bytes per update from the shapes: x and the time features read, the x_l / x_r rows written and read back, alpha,
    m and the entropy written and read back, the statistics read and written once per group present (they are in fact read and
    written once per chunk: stated next to the number); from those each launch's share of the 8 TB/s HBM bound;
  * wall time of evaluate_attention against evaluate_split over the same 20 batches (the set-up of tools/baseline_bench.py:
    model + historical average), alternating, one warm-up pass each.

    python tools/spatial_attention_bench.py [--out PREFIX] [--no-profile]     # writes PREFIX.json and PREFIX.txt
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

B, L_IN, C_IN, HEADS = 16, 48, 6, 2
HBM_BYTES_PER_S = 8e12
PROFILE_UPDATES = 5
CASES = [1, 12]
KERNELS = ("spatial_attn_rows_kernel", "spatial_attn_target_kernel", "spatial_attn_accumulate_kernel")


def algorithmic_bytes(E2, groups):
    G = B * L_IN
    rows = G * N * 2 * 24 * 4
    per_entry = G * E2 * HEADS * 4
    entropy = G * N * HEADS * 4
    stats = groups * (3 * E2 + N) * HEADS * 8
    return {KERNELS[0]: G * N * C_IN * 4 + G * 4 * 4 + rows,
            KERNELS[1]: rows + 2 * per_entry + entropy,
            KERNELS[2]: 2 * per_entry + entropy + 2 * stats}


def _model():
    import torch
    from oracle import ref_cpu as R
    from src.model.tec_mollm import TEC_MoLLM
    cfg = R.default_config(L_in=L_IN, L_out=L_OUT, num_nodes=N)
    torch.manual_seed(3)
    with torch.device("cuda"):
        return TEC_MoLLM(dict(cfg, include_wte=False, load_pretrained_gpt2=False, gat_graphs="per_timestep")).eval()


def kernels_only():
    """The child run under the profiler: per case one warm-up update and PROFILE_UPDATES more, cases in CASES order."""
    import torch
    from oracle import ref_cpu as R
    from tecmollm import AttentionStats, graph_groups_by_slot
    from tecmollm import graph as graph_
    from tecmollm.synthetic import synthetic_batch
    model = _model()
    ei = R.grid_graph()[0].cuda()
    x, tf, _ = synthetic_batch(B, L_IN, N, C_IN, L_OUT)
    x, tf = x.cuda(), tf.cuda()
    E2 = graph_.get(ei, N, x.device, 16).num_edges + N
    for G in CASES:
        st = AttentionStats(N, E2, G)
        ids = graph_groups_by_slot(tf) if G > 1 else None
        for _ in range(1 + PROFILE_UPDATES):
            st.update(model, x, tf, ei, ids)
        torch.cuda.synchronize()


def profile_kernels(timeout=540):
    """[{kernel: (updates, chunks, mean us per update, min, max)} per case] from a rocprofv3 run of `--kernels-only`."""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "attn", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, start, end from kernels order by start").fetchall()
    out = [dict() for _ in CASES]
    for kern in KERNELS:
        us = [(e - s) / 1e3 for name, s, e in rows if kern in name]
        per_case = len(us) // len(CASES)
        chunks = per_case // (1 + PROFILE_UPDATES)
        if chunks < 1 or chunks * (1 + PROFILE_UPDATES) * len(CASES) != len(us):
            raise RuntimeError(f"{kern}: {len(us)} launches do not split into {len(CASES)} cases of {1 + PROFILE_UPDATES} updates")
        for c in range(len(CASES)):
            mine = np.asarray(us[c * per_case:(c + 1) * per_case]).reshape(1 + PROFILE_UPDATES, chunks)[1:].sum(axis=1)
            out[c][kern] = (int(mine.size), chunks, float(mine.mean()), float(mine.min()), float(mine.max()))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_attention"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (kernel time: not measured)")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    kern = [] if a.no_profile else profile_kernels()                       # before this process opens the GPU
    import torch
    from oracle import ref_cpu as R
    from tecmollm import evaluate as E
    from tecmollm import evaluate_attention
    from tecmollm import graph as graph_
    if not torch.cuda.is_available():
        raise SystemExit("spatial_attention_bench.py measures on the GPU; none found")
    dev_name = torch.cuda.get_device_name(0)
    ei = R.grid_graph()[0].cuda()
    E2 = graph_.get(ei, N, ei.device, 16).num_edges + N
    lines, rows = [f"# {dev_name}; N = {N}, E'' = {E2}, L_in = {L_IN}, B = {B}, {B * L_IN} graphs per update, fp32"], []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    for G, per in zip(CASES, kern):
        nbytes = algorithmic_bytes(E2, G)
        for k in KERNELS:
            cnt, chunks, us, lo, hi = per[k]
            share = nbytes[k] / (us * 1e-6) / HBM_BYTES_PER_S
            rows.append(dict(kernel=k, groups=G, chunks=chunks, algorithmic_bytes=nbytes[k], us_per_update=us, us_min=lo,
                             us_max=hi, updates=cnt, algorithmic_GBps=nbytes[k] / us / 1e3, share_of_hbm_bound=share))
            say(f"{k}, {G} group(s): {us:.1f} us per update over {chunks} chunks (min {lo:.1f}, max {hi:.1f}; rocprofv3 kernel "
                f"trace, {cnt} updates), algorithmic {nbytes[k] / 1e6:.1f} MB -> {nbytes[k] / us / 1e3:.0f} GB/s = "
                f"{share:.3f} of the 8 TB/s HBM bound")
    if not kern:
        say("kernel time: not measured")
    model = _model()
    X, TF = split_arrays()
    ds = dataset(X, TF, L_IN)
    order = list(range(20 * B))
    runs = {"evaluate_split": lambda: E.evaluate_split(model, ds, ei, B, scaler=(20.0, 8.0), order=order),
            "evaluate_attention G=1": lambda: evaluate_attention(model, ds, ei, B, order=order),
            "evaluate_attention slot": lambda: evaluate_attention(model, ds, ei, B, groups="slot", order=order)}
    times = {k: [] for k in runs}
    for p in range(1 + a.passes):
        for k, fn in runs.items():
            s = wall(fn)
            if p:
                times[k].append(s)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    say(f"20 batches at B = {B}, L_in = {L_IN}, fp32, per-timestep graphs, median wall of {a.passes} alternating passes: "
        + ", ".join(f"{k} {v:.3f} s" for k, v in med.items())
        + f"; ratios to evaluate_split {med['evaluate_attention G=1'] / med['evaluate_split']:.3f} and "
        f"{med['evaluate_attention slot'] / med['evaluate_split']:.3f}  (evaluate_attention's wall includes compute(): the "
        f"statistics copied to the host and derived in numpy; all passes: {times})")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, E2=E2, kernel=rows,
                       attention_vs_split=dict(batches=20, B=B, L_in=L_IN, median_s=med, all_s=times)), f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
