"""Times of SarimaBaseline (src/models/baselines.py, csrc/sarima.hip) at the shapes it is used at.  Recorded, not gated: there
is no earlier device path to compare with, and no time was promised.

  * fit: the full training split, T = 4380 two-hourly steps, N = 2911, channel 0 of the resident (T, N * 6) split read in
    place, default orders (1,1,1)(1,1,1,12): device events around back-to-back tecm_sar_fit calls (five launches each), the
    wall time of SarimaBaseline.fit (+ the copy of theta, the numpy invertibility check, the second solve, the copies of
    the results), and how many nodes end with each status bit;
  * forecast: every stride-1 window of a full test split (T = 2208), L_in = 48 and 336, L_out = 12, one tecm_sar_forecast
    launch into a (windows, 12, N) buffer: device events, beside the window mean (tecm_window_baseline) over the same windows;
  * kernel times: a child run under `rocprofv3 --kernel-trace --stats` started before this process touches the GPU, first
    launch of every kernel dropped.

    python tools/sarima_bench.py [--out PREFIX] [--no-profile]             # writes PREFIX.json and PREFIX.txt
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
for _p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

T_TRAIN, T_TEST, H, W, CH, L_OUT = 4380, 2208, 41, 71, 6, 12
N = H * W
CASES = (48, 336)
PROFILE_LAUNCHES = 10


def split(T, seed):
    """(T, N, CH) fp32 on the host: channel 0 a TEC-like series (diurnal shape x slow amplitude + AR(1) noise), the rest noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    phase = rng.uniform(0, 2 * np.pi, N)[None, :]
    tec = (1.0 + 0.6 * np.sin(2 * np.pi * t / 12 + phase)) * 20.0 * (1.0 + 0.3 * np.sin(2 * np.pi * t / 327.0 + phase))
    noise, eps = np.zeros((T, N)), rng.standard_normal((T, N))
    for i in range(1, T):
        noise[i] = 0.7 * noise[i - 1] + eps[i]
    X = rng.standard_normal((T, N, CH)).astype(np.float32)
    X[:, :, 0] = (tec + 1.5 * noise).astype(np.float32)
    return X


class Work:
    def __init__(self):
        import torch
        from src.models.baselines import SarimaBaseline
        self.torch = torch
        self.train = torch.from_numpy(split(T_TRAIN, 0)).cuda()
        self.test = torch.from_numpy(split(T_TEST, 1)).cuda()
        self.sb = SarimaBaseline()
        self.series = self.train[:, :, 0]

    def fit_kernels(self):
        return self.sb.fit_device(self.series)

    def forecaster(self, L_in):
        S = T_TEST - L_in - L_OUT + 1
        starts = list(range(S))
        out = self.torch.empty(S, L_OUT, N, device="cuda")
        coef = self.sb._coef_on(self.test.device)
        return S, lambda: self.sb.forecast_series(self.test, starts, L_in, L_OUT, out=out, coef=coef)

    def mean_launch(self, L_in):
        import ctypes as C
        from tecmollm import _lib
        S = T_TEST - L_in - L_OUT + 1
        starts = self.torch.arange(S, dtype=self.torch.int64).cuda()
        out = self.torch.empty(S, N, device="cuda")
        desc = _lib.TecmWindowBaseline(X=self.test.data_ptr(), starts=starts.data_ptr(), starts_host_check=None, T=T_TEST, N=N,
                                       C=CH, channel=0, L_in=L_in, L_out=L_OUT, B=S, mode=_lib.TECM_BASELINE_MEAN, period=0,
                                       out=out.data_ptr(), o_stride_b=N, o_stride_h=0, o_stride_n=1)
        keep = (starts, out)
        return lambda: (_lib.check(_lib.lib().tecm_window_baseline(C.byref(desc), _lib.stream_ptr()), "mean"), keep)[0]


def kernels_only():
    w = Work()
    w.sb.fit(w.series)
    for _ in range(1 + PROFILE_LAUNCHES):
        w.fit_kernels()
    for L_in in CASES:
        _, run = w.forecaster(L_in)
        for _ in range(1 + PROFILE_LAUNCHES):
            run()
    w.torch.cuda.synchronize()


def profile_kernels(timeout=540):
    """{kernel name fragment: {grid blocks: (launches, mean us, min us, max us)}} from a rocprofv3 run of `--kernels-only`."""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "sarima", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, grid_x, workgroup_x, start, end from kernels order by start").fetchall()
    per = {}
    for name, gx, wx, s, e in rows:
        for frag in ("sar_autocov", "sar_levinson", "sar_gram_join", "sar_gram_kernel", "sar_solve", "sar_forecast"):
            if frag in name:
                per.setdefault(frag, {}).setdefault(gx // wx, []).append((e - s) / 1e3)
                break
    return {f: {b: (len(us) - 1, float(np.mean(us[1:])), float(np.min(us[1:])), float(np.max(us[1:])))
                for b, us in by.items() if len(us) > 1} for f, by in per.items()}


def event_time(torch, launch, min_seconds=0.25):
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    n = max(5, int(min_seconds / max((time.perf_counter() - t0) / 3, 1e-6)) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3, n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sarima"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (kernel times: not measured)")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    kern, why = {}, "skipped (--no-profile)"
    if not a.no_profile:
        try:
            kern = profile_kernels()                                       # before this process opens the GPU
        except Exception as exc:                                           # recorded, not fatal: the event times stand alone
            why = f"failed: {exc}"
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sarima_bench.py measures on the GPU; none found")
    dev_name = torch.cuda.get_device_name(0)
    lines, rec = [f"# {dev_name}; N = {N}, C = {CH}, orders (1,1,1)(1,1,1,12), long AR 26, L_out = {L_OUT}, stride 1"], {}

    def say(s):
        lines.append(s)
        print(s, flush=True)
    w = Work()
    fit_us, n = event_time(torch, w.fit_kernels)
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w.sb.fit(w.series)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    st = w.sb.status_
    rec["fit"] = dict(T=T_TRAIN, call_us_events=fit_us, event_calls=n, fit_wall_s=sorted(walls)[1],
                      series_bytes=T_TRAIN * N * 4, touched_bytes=T_TRAIN * N * 4 * CH,
                      degenerate=int((st & 1 != 0).sum()), nonfinite=int((st & 2 != 0).sum()), ma_dropped=int((st & 4 != 0).sum()))
    say(f"fit, training split T = {T_TRAIN} (series {T_TRAIN * N * 4 / 1e6:.1f} MB, {T_TRAIN * N * 4 * CH / 1e6:.0f} MB of touched lines):")
    say(f"  tecm_sar_fit, five launches, {(N + 63) // 64} node tiles x {-(-(T_TRAIN - 13) // 1024)} chunks of time "
        f"(device events, {n} back-to-back calls): {fit_us:.1f} us")
    say(f"  SarimaBaseline.fit wall (+ theta to the host, invertibility check, second solve, results to the host): "
        f"{sorted(walls)[1] * 1e3:.1f} ms;  status: {rec['fit']['degenerate']} degenerate, {rec['fit']['nonfinite']} non-finite, "
        f"{rec['fit']['ma_dropped']} of {N} nodes without MA part")
    for frag in ("sar_autocov", "sar_levinson", "sar_gram_kernel", "sar_gram_join", "sar_solve"):
        for blocks, (cnt, us, lo, hi) in sorted(kern.get(frag, {}).items()):
            say(f"    {frag} ({blocks} node tiles; rocprofv3 kernel trace, {cnt} launches): {us:.1f} us (min {lo:.1f}, max {hi:.1f})")
    rec["forecast"] = []
    for L_in in CASES:
        S, run = w.forecaster(L_in)
        us, n = event_time(torch, run)
        mean_us, n2 = event_time(torch, w.mean_launch(L_in))
        algo = S * L_in * N * 4
        row = dict(L_in=L_in, windows=S, call_us_events=us, event_calls=n, window_mean_call_us_events=mean_us,
                   algorithmic_bytes=algo, output_bytes=S * L_OUT * N * 4)
        say(f"forecast L_in {L_in:>3}: {S} windows x {N} nodes, {algo / 1e9:.3f} GB of window values, {S * L_OUT * N * 4 / 1e6:.0f} MB written")
        say(f"  tecm_sar_forecast (device events, {n} back-to-back launches): {us:.1f} us = {algo / us / 1e3:.0f} GB/s on the window "
            f"values;  tecm_window_baseline MEAN over the same windows, same method: {mean_us:.1f} us")
        for blocks, (cnt, kus, lo, hi) in sorted(kern.get("sar_forecast", {}).items()):
            if blocks == S * ((N + 63) // 64):
                row.update(kernel_us=kus, kernel_us_min=lo, kernel_us_max=hi)
                say(f"  kernel time (rocprofv3 kernel trace, {cnt} launches): {kus:.1f} us (min {lo:.1f}, max {hi:.1f})")
        rec["forecast"].append(row)
    if not kern:
        say(f"kernel times (rocprofv3): not measured, {why}")
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, **rec, kernels={k: {str(b): v for b, v in by.items()} for k, by in kern.items()}), f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
