"""Cost of event verification at the test split's batch shape, B = 16, L_out = 12, N = 2911 = 41 x 71, Q = 4 thresholds
relative to a (N, 12) climatology (slots in use).  Recorded, not gated.

  * kernel times of event_hist_kernel for K = 1 (the model's permuted output view) and K = 16 (member-major), each with 1
    and 4 groups, and of event_fss_kernel at W = 4 widths (1, 3, 5, 9) with 1 and 4 groups: a run of its own under
    `rocprofv3 --kernel-trace --stats` (a child process started before this one touches the GPU), read from the trace
    database, first launch of every case dropped;
  * algorithmic bytes: the histogram reads (K + 1) operands of B*H*N*4 B and Q*B*H*N*4 B of thresholds (a slot per
    (sample, horizon)) and reads and writes the G*Q*H*(K+1)*2*N*4 B of counts; the FSS reads two operands and the thresholds
    and writes G*Q*H*W*3*8 B;
  * wall time of `evaluate_events` (model + historical average, K = 1, with the grid) against `evaluate_maps` over the same
    20 batches at L_in = 48 in the same run, median of `--passes` alternating passes after one warm-up pass;
  * for context, the numpy restatement (tests/events_ref.py) of the histogram and of the FSS sums of ONE batch on the host.

    python tools/events_bench.py [--out PREFIX] [--no-profile]           # writes PREFIX.json and PREFIX.txt
"""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tec-mollm_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

from baseline_bench import L_OUT, N, dataset, split_arrays, wall  # noqa: E402

B = 16
Q = 4
GRID = (41, 71)
SCALES = (1, 3, 5, 9)
SCALER = (20.0, 8.0)
REL = (0.3, -0.3, 0.1, -0.1)
HIST_CASES = ((1, 1), (1, 4), (16, 1), (16, 4))          # (members, groups)
FSS_CASES = (1, 4)                                       # groups
PROFILE_LAUNCHES = 10


def thresholds():
    from tecmollm.events import EventThresholds
    clim = SCALER[0] + 0.5 * SCALER[1] * np.random.default_rng(0).standard_normal((N, 12))
    return EventThresholds.relative(clim, rel=REL)


def hist_bytes(K, G):
    return (K + 1) * B * L_OUT * N * 4 + Q * B * L_OUT * N * 4 + 2 * G * Q * L_OUT * (K + 1) * 2 * N * 4


def fss_bytes(G):
    return 2 * B * L_OUT * N * 4 + Q * B * L_OUT * N * 4 + G * Q * L_OUT * len(SCALES) * 3 * 8


def operands(K):
    import torch
    g = torch.Generator(device="cuda").manual_seed(K)
    y = torch.randn(B, L_OUT, N, 1, device="cuda", generator=g)
    if K == 1:
        p = torch.randn(B, N, L_OUT, device="cuda", generator=g).permute(0, 2, 1).unsqueeze(-1)
    else:
        p = torch.randn(K, B, L_OUT, N, device="cuda", generator=g)
    slots = torch.randint(0, 12, (B, L_OUT), device="cuda", generator=g, dtype=torch.int32)
    return p, y, slots


def kernels_only():
    """The child run under the profiler: per case one warm-up update and PROFILE_LAUNCHES more, histogram cases first."""
    import torch
    from src.evaluation.metrics import EventMetrics
    th = thresholds()
    for K, G in HIST_CASES:
        p, y, slots = operands(K)
        em = EventMetrics(L_OUT, N, th, G, SCALER, K)
        ids = (torch.arange(B, device="cuda", dtype=torch.int32) % G) if G > 1 else None
        for _ in range(1 + PROFILE_LAUNCHES):
            em.update(p, y, ids, slots)
        torch.cuda.synchronize()
    for G in FSS_CASES:
        p, y, slots = operands(1)
        em = EventMetrics(L_OUT, N, th, G, SCALER, 1, grid=GRID, scales=SCALES)
        ids = (torch.arange(B, device="cuda", dtype=torch.int32) % G) if G > 1 else None
        for _ in range(1 + PROFILE_LAUNCHES):
            em.update(p, y, ids, slots)
        torch.cuda.synchronize()


def profile_kernels(timeout=420):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "events", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, start, end from kernels order by start").fetchall()
    per = 1 + PROFILE_LAUNCHES
    hist = [(e - s) / 1e3 for name, s, e in rows if "event_hist_kernel" in name]
    fss = [(e - s) / 1e3 for name, s, e in rows if "event_fss_kernel" in name]
    # the FSS cases launch the histogram kernel too: the timed histogram launches are the first ones
    if len(hist) != per * (len(HIST_CASES) + len(FSS_CASES)) or len(fss) != per * len(FSS_CASES):
        raise RuntimeError(f"unexpected launch counts: {len(hist)} histogram, {len(fss)} FSS")
    summary = lambda u: (len(u), float(np.mean(u)), float(np.min(u)), float(np.max(u)))
    out = {("hist",) + case: summary(hist[c * per + 1:(c + 1) * per]) for c, case in enumerate(HIST_CASES)}
    out.update({("fss", G): summary(fss[c * per + 1:(c + 1) * per]) for c, G in enumerate(FSS_CASES)})
    return out


def host_restatement():
    """Seconds the numpy restatement takes for the histogram (K = 1) and for the FSS sums of one batch."""
    from tests import events_ref as ER
    th = thresholds()
    rng = np.random.default_rng(1)
    p = rng.standard_normal((B, L_OUT, N)).astype(np.float32)
    y = rng.standard_normal((B, L_OUT, N)).astype(np.float32)
    slots = rng.integers(0, 12, size=(B, L_OUT))
    t0 = time.perf_counter()
    ER.accumulate_hist(np.zeros((1, Q, L_OUT, 2, 2, N), dtype=np.int64), p[None], y, th.values, th.strides, th.dirs, None, SCALER,
                       slots, 12)
    t1 = time.perf_counter()
    ER.accumulate_fss(np.zeros((1, Q, L_OUT, len(SCALES), 3), dtype=np.int64), p, y, th.values, th.strides, th.dirs, SCALES, GRID,
                      None, SCALER, slots, 12)
    return t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (kernel time: not measured)")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    kern = {} if a.no_profile else profile_kernels()                       # before this process opens the GPU
    import torch
    from tecmollm import evaluate as E
    from tecmollm import events as EV
    if not torch.cuda.is_available():
        raise SystemExit("events_bench.py measures on the GPU; none found")
    dev_name = torch.cuda.get_device_name(0)
    lines, rows = [f"# {dev_name}; N = {N} = {GRID[0]} x {GRID[1]}, L_out = {L_OUT}, B = {B}, Q = {Q}; python tools/events_bench.py"
                   + (" --no-profile" if a.no_profile else "") + f" --passes {a.passes}"], []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    for key, (cnt, us, lo, hi) in kern.items():
        if key[0] == "hist":
            name, what, nbytes = "event_hist_kernel", f"K = {key[1]}, {key[2]} group(s)", hist_bytes(key[1], key[2])
        else:
            name, what, nbytes = "event_fss_kernel", f"W = {len(SCALES)}, {key[1]} group(s)", fss_bytes(key[1])
        rows.append(dict(kernel=name, case=list(key[1:]), algorithmic_bytes=nbytes, kernel_us=us, kernel_us_min=lo,
                         kernel_us_max=hi, launches=cnt, algorithmic_GBps=nbytes / us / 1e3))
        say(f"{name}, {what}: {us:.1f} us (min {lo:.1f}, max {hi:.1f}; rocprofv3 kernel trace, {cnt} launches), algorithmic "
            f"{nbytes / 1e6:.2f} MB -> {nbytes / us / 1e3:.0f} GB/s")
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
    th = thresholds()
    runs = {"evaluate_maps": lambda: E.evaluate_maps(model, ds, ei, B, scaler=SCALER, order=order),
            "evaluate_events": lambda: EV.evaluate_events(model, ds, ei, B, th, scaler=SCALER, order=order, grid=GRID,
                                                          scales=SCALES)}
    times = {k: [] for k in runs}
    for p in range(1 + a.passes):
        for k, fn in runs.items():
            s = wall(fn)
            if p:
                times[k].append(s)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    ratio = med["evaluate_events"] / med["evaluate_maps"]
    say(f"20 batches at B = {B}, L_in = 48, fp32, model + historical average, K = 1, grid {GRID}, W = {len(SCALES)}, median wall "
        f"of {a.passes} alternating passes: " + ", ".join(f"{k} {v:.3f} s" for k, v in med.items())
        + f"; evaluate_events / evaluate_maps = {ratio:.3f}  (all passes: {times})")
    h_s, f_s = host_restatement()
    say(f"numpy restatement of one batch on the host (tests/events_ref.py): histogram K = 1 {h_s:.2f} s, FSS sums W = "
        f"{len(SCALES)} {f_s:.2f} s")
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, kernel=rows, events_vs_maps=dict(batches=20, B=B, L_in=48, median_s=med, all_s=times,
                                                                        ratio=ratio),
                       host_restatement_s=dict(histogram=h_s, fss=f_s)), f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
