"""Cost of the conformal intervals at the full split's size, S = 2149 windows, L_out = 12, N = 2911 (a score store of
2149 x 34932 float32 = 300 MB), next to the same quantiles by `torch.sort` / `torch.kthvalue` on the same store.  Recorded,
not gated.

  * kernel times of conformal_scores_kernel and interval_stats_kernel (one batch of B = 16, the model's permuted output
    layout against the dataset's target layout) and of column_select_kernel on the whole store, for (G, Q) = (1, 1), (4, 1)
    and (1, 2): a run of its own under `rocprofv3 --kernel-trace --stats` (a child process started before this one touches
    the GPU), read from the trace database, first launch of every case dropped;
  * algorithmic bytes: scores 3 operands of B*H*N*4 B (two reads, one write); statistics two reads of that size, the
    quantiles and a read and a write of G*H*N*6*8 B; selection four passes of Q * S*C*4 B (every pass reads every row of
    every group once per rank; a row of another group is not loaded);
  * wall time of `ConformalCalibrator.fit` end to end (bincount, host synchronisation, ranks, selection, quantiles to the
    host), of `torch.sort(store, dim=0)` plus the row of the rank, and of `torch.kthvalue(store, k, dim=0)`, each ending in
    a device synchronise, median of `--passes` alternating passes after one warm-up pass.

    python tools/conformal_bench.py [--out PREFIX] [--no-profile]           # writes PREFIX.json and PREFIX.txt
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

S = 2149
B = 16
C = L_OUT * N
ALPHA = 0.1
SELECT_CASES = ((1, 1), (4, 1), (1, 2))          # (groups, ranks per group)
PROFILE_LAUNCHES = 10
SCALER = (20.0, 8.0)
KERNELS = ("conformal_scores_kernel", "interval_stats_kernel", "column_select_kernel")


def batch_bytes(kernel, G=1):
    if kernel == "conformal_scores_kernel":
        return 3 * B * C * 4
    return 2 * B * C * 4 + C * 4 + 2 * G * C * 6 * 8


def select_bytes(Q):
    return 4 * Q * S * C * 4


def filled_store(G):
    """A calibrator whose store holds S rows of |N(0, 1)| scores (written by the score kernel), ids spread over G groups."""
    import torch
    from tecmollm import ConformalCalibrator
    gen = torch.Generator(device="cuda").manual_seed(G)
    cal = ConformalCalibrator(L_OUT, N, S, G, None, "absolute")
    for a in range(0, S, 256):
        n = min(256, S - a)
        truth = torch.randn(n, L_OUT, N, device="cuda", generator=gen)
        ids = (torch.arange(a, a + n, device="cuda") % G).to(torch.int32)
        cal.update(torch.zeros(n, L_OUT, N, device="cuda"), truth, ids)
    return cal


def select_launch(cal, G, Q):
    import torch
    from tecmollm import devcheck, ops
    counts = np.bincount(np.arange(S) % G, minlength=G)
    ranks = torch.from_numpy(np.array([[int(n * (0.9 if q == Q - 1 else 0.05)) for q in range(Q)] for n in counts],
                                      dtype=np.int32)).cuda()
    ids, err = cal.groups[:S], devcheck.error_word("cuda").ptr()
    return lambda: ops.column_select(cal.scores[:S], ranks, ids, err)


def kernels_only():
    """The child run under the profiler: per case one warm-up launch and PROFILE_LAUNCHES more, in KERNELS order."""
    import torch
    from src.evaluation.metrics import IntervalMetrics
    from tecmollm import ConformalCalibrator
    torch.manual_seed(0)
    pred = torch.randn(B, N, L_OUT, device="cuda").permute(0, 2, 1).unsqueeze(-1)       # the model's output view
    y = torch.randn(B, L_OUT, N, 1, device="cuda")
    cal = ConformalCalibrator(L_OUT, N, B, 1, SCALER, "absolute")
    for _ in range(1 + PROFILE_LAUNCHES):
        cal.reset()
        cal.update(pred, y)
    torch.cuda.synchronize()
    im = IntervalMetrics(L_OUT, N, 1, SCALER, ALPHA, "absolute")
    q = (None, torch.rand(1, L_OUT, N, device="cuda") * 10)
    for _ in range(1 + PROFILE_LAUNCHES):
        im.update(pred, y, q)
    torch.cuda.synchronize()
    for G, Q in SELECT_CASES:
        cal = filled_store(G)
        torch.cuda.synchronize()
        launch = select_launch(cal, G, Q)
        for _ in range(1 + PROFILE_LAUNCHES):
            launch()
        torch.cuda.synchronize()
        del cal, launch


def profile_kernels(timeout=600):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "conformal", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, start, end from kernels order by start").fetchall()
    out = {}
    per = 1 + PROFILE_LAUNCHES
    stats = [(e - s) / 1e3 for name, s, e in rows if "interval_stats_kernel" in name]
    select = [(e - s) / 1e3 for name, s, e in rows if "column_select_kernel" in name]
    # the stores of the selection cases are filled by the score kernel too: the timed batch launches are the first `per`
    scores = [(e - s) / 1e3 for name, s, e in rows if "conformal_scores_kernel" in name][:per]
    if len(scores) != per or len(stats) != per or len(select) != per * len(SELECT_CASES):
        raise RuntimeError(f"unexpected launch counts: {len(scores)} scores, {len(stats)} statistics, {len(select)} selections")
    summary = lambda u: (len(u), float(np.mean(u)), float(np.min(u)), float(np.max(u)))
    out["conformal_scores_kernel"] = summary(scores[1:])
    out["interval_stats_kernel"] = summary(stats[1:])
    for c, case in enumerate(SELECT_CASES):
        out[case] = summary(select[c * per + 1:(c + 1) * per])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conformal"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (kernel time: not measured)")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    kern = {} if a.no_profile else profile_kernels()                       # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("conformal_bench.py measures on the GPU; none found")
    from tecmollm import conformal_ranks
    dev_name = torch.cuda.get_device_name(0)
    lines, rows = [f"# {dev_name}; S = {S}, L_out = {L_OUT}, N = {N}, store {S * C * 4 / 1e6:.0f} MB; "
                   f"python tools/conformal_bench.py" + (" --no-profile" if a.no_profile else "") + f" --passes {a.passes}"], []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    for name in KERNELS[:2]:
        if name in kern:
            cnt, us, lo, hi = kern[name]
            nbytes = batch_bytes(name)
            rows.append(dict(kernel=name, B=B, algorithmic_bytes=nbytes, kernel_us=us, kernel_us_min=lo, kernel_us_max=hi,
                             launches=cnt, algorithmic_GBps=nbytes / us / 1e3))
            say(f"{name}, B = {B}: {us:.1f} us (min {lo:.1f}, max {hi:.1f}; rocprofv3 kernel trace, {cnt} launches), "
                f"algorithmic {nbytes / 1e6:.2f} MB -> {nbytes / us / 1e3:.0f} GB/s")
    for G, Q in SELECT_CASES:
        if (G, Q) in kern:
            cnt, us, lo, hi = kern[(G, Q)]
            nbytes = select_bytes(Q)
            rows.append(dict(kernel="column_select_kernel", G=G, Q=Q, algorithmic_bytes=nbytes, bytes_per_pass=nbytes // 4,
                             kernel_us=us, kernel_us_min=lo, kernel_us_max=hi, launches=cnt, algorithmic_GBps=nbytes / us / 1e3))
            say(f"column_select_kernel, G = {G}, Q = {Q}: {us:.1f} us (min {lo:.1f}, max {hi:.1f}; rocprofv3 kernel trace, {cnt} "
                f"launches), algorithmic 4 passes x {nbytes / 4e6:.0f} MB = {nbytes / 1e6:.0f} MB -> {nbytes / us / 1e3:.0f} GB/s")
    if not kern:
        say("kernel time: not measured")
    cal = filled_store(1)
    store = cal.scores[:S]
    k, = conformal_ranks(S, ALPHA)
    got = {}

    def fit():
        got["fit"] = cal.fit(ALPHA).q_hi.reshape(-1)

    def by_sort():
        got["sort"] = torch.sort(store, dim=0).values[k - 1].cpu().numpy()

    def by_kthvalue():
        got["kthvalue"] = torch.kthvalue(store, k, dim=0).values.cpu().numpy()
    runs = {"fit": fit, "torch.sort": by_sort, "torch.kthvalue": by_kthvalue}
    times = {name: [] for name in runs}
    for p in range(1 + a.passes):
        for name, fn in runs.items():
            s = wall(fn)
            if p:
                times[name].append(s)
    same = bool(np.array_equal(got["fit"], got["sort"]) and np.array_equal(got["fit"], got["kthvalue"]))
    med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
    say(f"rank {k} of {S} in each of {C} cells, one group: ConformalCalibrator.fit end to end {med['fit'] * 1e3:.2f} ms, "
        f"torch.sort + row {med['torch.sort'] * 1e3:.2f} ms, torch.kthvalue {med['torch.kthvalue'] * 1e3:.2f} ms (host clock "
        f"around a synchronise, quantiles copied to the host in all three); identical quantiles: {same}; median of {a.passes} "
        "alternating passes")
    say(f"all passes, seconds: {times}")
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, S=S, L_out=L_OUT, N=N, kernel=rows, wall=dict(rank=k, median_s=med, all_s=times,
                                                                                      identical=same)), f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
