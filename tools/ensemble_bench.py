"""Cost of the ensemble scores (EnsembleMetrics / tecm_ensemble_stats) at the full grid, N = 2911, L_out = 12, B = 16, for
K = 8, 16 and 32 members, next to the K stochastic forwards an update follows.  Recorded, not gated.

  * kernel time of ensemble_stats_kernel: a run of its own under `rocprofv3 --kernel-trace --stats` (a child process started
    before this one touches the GPU), read from the trace database, first launch of every case dropped.  Members
    node-contiguous (what `ensemble_members` returns), the dataset's target layout, one group, no per-sample outputs;
  * algorithmic bytes per update: K + 1 operands of S*H*I*4 B plus a read and a write of H*I*(9*8 + (K+1)*4) B of statistics
    and rank counts;
  * wall time of `ensemble_members` (K training-mode forwards at B = 16, L_in = 48, fp32, with the transposing copies) and
    of the update with its `mean_raw` output, each ending in a device synchronise, median of `--passes` alternating passes
    after one warm-up pass.

    python tools/ensemble_bench.py [--out PREFIX] [--no-profile]           # writes PREFIX.json and PREFIX.txt
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

from baseline_bench import L_OUT, N, wall  # noqa: E402

B = 16
L_IN = 48
MEMBERS = (8, 16, 32)
PROFILE_LAUNCHES = 20
SCALER = (20.0, 8.0)


def algorithmic_bytes(K, G=1):
    return (K + 1) * B * L_OUT * N * 4 + 2 * G * L_OUT * N * (9 * 8 + (K + 1) * 4)


def kernels_only():
    """The child run under the profiler: per K one warm-up update and PROFILE_LAUNCHES more, in MEMBERS order."""
    import torch
    from src.evaluation.metrics import EnsembleMetrics
    torch.manual_seed(0)
    y = torch.randn(B, L_OUT, N, 1, device="cuda")
    for K in MEMBERS:
        mem = torch.randn(K, B, L_OUT, N, device="cuda")
        em = EnsembleMetrics(L_OUT, N, K, 1, SCALER, 1)
        for _ in range(1 + PROFILE_LAUNCHES):
            em.update(mem, y)
        torch.cuda.synchronize()


def profile_kernels(timeout=420):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "ensemble", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, start, end from kernels order by start").fetchall()
    us = [(e - s) / 1e3 for name, s, e in rows if "ensemble_stats_kernel" in name]
    if len(us) != len(MEMBERS) * (1 + PROFILE_LAUNCHES):
        raise RuntimeError(f"expected {len(MEMBERS) * (1 + PROFILE_LAUNCHES)} launches of ensemble_stats_kernel, saw {len(us)}")
    out = []
    for c in range(len(MEMBERS)):
        u = us[c * (1 + PROFILE_LAUNCHES) + 1:(c + 1) * (1 + PROFILE_LAUNCHES)]
        out.append((len(u), float(np.mean(u)), float(np.min(u)), float(np.max(u))))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (kernel time: not measured)")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    kern = [] if a.no_profile else profile_kernels()                       # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench.py measures on the GPU; none found")
    from oracle import ref_cpu as R
    from src.evaluation.metrics import EnsembleMetrics
    from src.model.tec_mollm import TEC_MoLLM
    from tecmollm import ensemble_members
    dev_name = torch.cuda.get_device_name(0)
    lines, rows = [f"# {dev_name}; N = {N}, L_out = {L_OUT}, B = {B}; python tools/ensemble_bench.py"
                   + (" --no-profile" if a.no_profile else "") + f" --passes {a.passes}"], []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    for K, k in zip(MEMBERS, kern):
        cnt, us, lo, hi = k
        nbytes = algorithmic_bytes(K)
        rows.append(dict(members=K, algorithmic_bytes=nbytes, kernel_us=us, kernel_us_min=lo, kernel_us_max=hi, launches=cnt,
                         algorithmic_GBps=nbytes / us / 1e3))
        say(f"ensemble_stats_kernel, K = {K}: {us:.1f} us (min {lo:.1f}, max {hi:.1f}; rocprofv3 kernel trace, {cnt} launches), "
            f"algorithmic {nbytes / 1e6:.2f} MB -> {nbytes / us / 1e3:.0f} GB/s")
    if not kern:
        say("kernel time: not measured")
    cfg = R.default_config(L_in=L_IN, L_out=L_OUT, num_nodes=N)
    torch.manual_seed(3)
    with torch.device("cuda"):
        model = TEC_MoLLM(dict(cfg, include_wte=False, load_pretrained_gpt2=False)).eval()
    x, tf, y = R.synthetic_batch(B, L_IN, N, cfg["spatial_in_channels_base"], L_OUT, seed=1)
    x, y = x.cuda(), y.cuda()
    tf = tf[:, :, 0, :].contiguous().cuda().unsqueeze(-2).expand(B, L_IN, N, 4)
    ei = R.grid_graph()[0].cuda()
    state = {}
    runs = {}
    for K in MEMBERS:
        em = EnsembleMetrics(L_OUT, N, K, 1, SCALER, 1)

        def forwards(K=K):
            state[K] = ensemble_members(model, x, tf, ei, K, seed=0)

        def update(K=K, em=em):
            em.update(state[K], y, outputs=("mean_raw",))
        runs[f"K={K} forwards"] = forwards
        runs[f"K={K} update"] = update
    times = {k: [] for k in runs}
    for p in range(1 + a.passes):
        for k, fn in runs.items():
            s = wall(fn)
            if p:
                times[k].append(s)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    for K in MEMBERS:
        f, u = med[f"K={K} forwards"], med[f"K={K} update"]
        say(f"K = {K}, B = {B}, L_in = {L_IN}, fp32: {K} training-mode forwards {f * 1e3:.1f} ms, one update with mean_raw "
            f"{u * 1e3:.3f} ms (host clock around a synchronise: launch overhead included), update / forwards = {u / f:.5f}; "
            f"median of {a.passes} alternating passes")
    say(f"all passes, seconds: {times}")
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, kernel=rows, wall=dict(B=B, L_in=L_IN, median_s=med, all_s=times)), f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
