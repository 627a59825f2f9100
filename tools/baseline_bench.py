"""Times of the evaluation baselines (tecmollm/evaluate.py) on a full test split: T = 2208, N = 2911, C = 6, every stride-1
window, L_in = 48 and 336.  Recorded, not gated: there is no earlier device path to compare with.

For the MEAN baseline (tecm_window_baseline, all windows in one launch, one value per (window, node)):
  * kernel time: a run of its own under `rocprofv3 --kernel-trace --stats` (a child process started before this one touches
    the GPU), read from the trace database, first launch of every case dropped;
  * call time: device events around back-to-back launches filling a window of at least 0.2 s, after warm-up;
  * algorithmic bytes = windows x L_in x N x 4 (the values that enter the sums) and touched bytes = x C (the stride-C channel
    read pulls whole lines, so every channel's bytes move), and the rate on each, named as such;
  * the wall time of get_baseline_predictions (kernel + the one copy of (windows, H, W, 12) to the host);
  * the reference's host loop (test.py:53-66) restated in numpy on the same box, timed over --host-windows windows
    and scaled to all windows (the scaled figure is labelled as scaled).
Then the wall time of evaluate_split (model + historical average) against loop.validate over the same 20 batches at B = 16
(L_in = 48, fp32, 3 GPT-2 blocks), alternating, one warm-up pass each.

    python tools/baseline_bench.py [--out PREFIX] [--no-profile]             # writes PREFIX.json and PREFIX.txt
"""
import argparse
import ctypes as C
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

T, H, W, CH, L_OUT = 2208, 41, 71, 6, 12
N = H * W
CASES = (48, 336)
PROFILE_LAUNCHES = 20


def split_arrays(seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, H, W, CH), dtype=np.float32)
    t = np.arange(T)
    TF = np.stack([t % 12, t % 366, np.zeros(T), (t // 30) % 4], 1).astype(np.float32)
    return X, TF


def dataset(X, TF, L_in):
    import torch
    from src.data.dataset import SlidingWindowSamplerDataset
    Y = torch.zeros(T, H, W, L_OUT)
    Y[..., :] = torch.from_numpy(X[..., 0:1])
    return SlidingWindowSamplerDataset.from_tensors(torch.from_numpy(X), Y, torch.from_numpy(TF), L_in, L_OUT, device="cuda",
                                                    mode="test")


class MeanLaunch:
    """One prepared tecm_window_baseline call over every window of `ds` (the work window_baseline does per call, without
    its host-side set-up)."""

    def __init__(self, ds):
        import torch
        from tecmollm import _lib
        self.S = len(ds)
        self.host = torch.tensor(ds.sample_indices, dtype=torch.int64)
        self.starts = self.host.cuda()
        self.out = torch.empty(self.S, N, device="cuda")
        self.desc = _lib.TecmWindowBaseline(X=ds.X.data_ptr(), starts=self.starts.data_ptr(), starts_host_check=None, T=T, N=N,
                                            C=CH, channel=0, L_in=ds.L_in, L_out=L_OUT, B=self.S,
                                            mode=_lib.TECM_BASELINE_MEAN, period=0, out=self.out.data_ptr(), o_stride_b=N,
                                            o_stride_h=0, o_stride_n=1)
        self.fn, self.check, self.stream = _lib.lib().tecm_window_baseline, _lib.check, _lib.stream_ptr()

    def __call__(self):
        self.check(self.fn(C.byref(self.desc), self.stream), "tecm_window_baseline")


def kernels_only():
    """The child run under the profiler: per case one warm-up launch and PROFILE_LAUNCHES more."""
    import torch
    X, TF = split_arrays()
    for L_in in CASES:
        launch = MeanLaunch(dataset(X, TF, L_in))
        for _ in range(1 + PROFILE_LAUNCHES):
            launch()
        torch.cuda.synchronize()


def profile_kernels(timeout=420):
    """{windows: (launches, mean us, min us, max us)} of window_baseline_kernel from a rocprofv3 run of `--kernels-only`."""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "baselines", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, grid_x, workgroup_x, start, end from kernels order by start").fetchall()
    per = {}
    for name, gx, wx, s, e in rows:
        if "window_baseline_kernel" in name:
            per.setdefault(gx // wx, []).append((e - s) / 1e3)
    out = {}
    tiles = (N + 255) // 256
    for blocks, us in per.items():
        us = us[1:]                                                       # the warm-up launch
        out[blocks // tiles] = (len(us), float(np.mean(us)), float(np.min(us)), float(np.max(us)))
    return out


def event_time(launch, min_seconds=0.25):
    import torch
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    n = max(10, int(min_seconds / max((time.perf_counter() - t0) / 5, 1e-6)) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        launch()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    return ms / n * 1e3, n, ms / 1e3


def host_loop(X, L_in, windows):
    """test.py:53-66 restated: per sample a time average of channel 0 of its window, repeated over the horizons."""
    Xt = X                                                                 # (T, H, W, C) on the host, as the reference holds it
    t0 = time.perf_counter()
    preds = []
    for a in range(windows):
        avg = np.mean(Xt[a:a + L_in][:, :, :, 0:1], axis=0, keepdims=True)
        preds.append(np.repeat(avg, L_OUT, axis=0).transpose(1, 2, 0, 3).squeeze(-1))
    out = np.array(preds)
    return time.perf_counter() - t0, out


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_baselines"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (kernel time: not measured)")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--host-windows", type=int, default=128)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    kern = {} if a.no_profile else profile_kernels()                       # before this process opens the GPU
    import torch
    from tecmollm import evaluate as E
    from tecmollm.loop import validate
    if not torch.cuda.is_available():
        raise SystemExit("baseline_bench.py measures on the GPU; none found")
    dev_name = torch.cuda.get_device_name(0)
    X, TF = split_arrays()
    rows, lines = [], [f"# {dev_name}; split T = {T}, N = {N}, C = {CH}, L_out = {L_OUT}, stride 1"]

    def say(s):
        lines.append(s)
        print(s, flush=True)
    for L_in in CASES:
        ds = dataset(X, TF, L_in)
        launch = MeanLaunch(ds)
        S = launch.S
        algo, touched = S * L_in * N * 4, S * L_in * N * 4 * CH
        call_us, n, window_s = event_time(launch)
        gp = [wall(lambda: E.get_baseline_predictions(ds, L_in, L_OUT)) for _ in range(1 + a.passes)][1:]
        hw = min(a.host_windows, S)
        host_s, host_out = host_loop(X, L_in, hw)
        same = bool(np.array_equal(E.get_baseline_predictions(ds, L_in, L_OUT)[:hw], host_out))
        row = dict(L_in=L_in, windows=S, algorithmic_bytes=algo, touched_bytes=touched, call_us_events=call_us,
                   event_launches=n, event_window_s=window_s, get_baseline_predictions_wall_s=sorted(gp)[len(gp) // 2],
                   host_loop_windows=hw, host_loop_s=host_s, host_loop_scaled_to_all_windows_s=host_s * S / hw,
                   bit_equal_to_host_loop=same)
        say(f"MEAN L_in {L_in:>3}: {S} windows, algorithmic {algo / 1e9:.3f} GB, touched {touched / 1e9:.3f} GB")
        if S in kern:
            cnt, us, lo, hi = kern[S]
            row.update(kernel_us=us, kernel_us_min=lo, kernel_us_max=hi, kernel_launches=cnt,
                       algorithmic_GBps=algo / us / 1e3, touched_GBps=touched / us / 1e3)
            say(f"  kernel time (rocprofv3 kernel trace, {cnt} launches): {us:.1f} us (min {lo:.1f}, max {hi:.1f}) -> "
                f"{algo / us / 1e3:.0f} GB/s on the algorithmic bytes, {touched / us / 1e3:.0f} GB/s on the touched bytes")
        else:
            say("  kernel time: not measured")
        say(f"  call time (device events, {n} back-to-back launches, {window_s:.2f} s): {call_us:.1f} us")
        say(f"  get_baseline_predictions wall (kernel + one copy of {S * N * L_OUT * 4 / 1e6:.0f} MB to the host): "
            f"{row['get_baseline_predictions_wall_s'] * 1e3:.1f} ms")
        say(f"  numpy restatement of the host loop: {host_s:.3f} s for {hw} windows = {host_s / hw * 1e3:.2f} ms per window, "
            f"{host_s * S / hw:.1f} s scaled to all {S} windows; same bits as the device: {same}")
        rows.append(row)
        del ds, launch
    # ---------------------------------------------------------------- evaluate_split against validate
    from oracle import ref_cpu as R
    from src.model.tec_mollm import TEC_MoLLM
    cfg = R.default_config(L_in=48, L_out=L_OUT, num_nodes=N)
    torch.manual_seed(3)
    with torch.device("cuda"):
        model = TEC_MoLLM(dict(cfg, include_wte=False, load_pretrained_gpt2=False)).eval()
    ds = dataset(X, TF, 48)
    ei = R.grid_graph()[0].cuda()
    order = list(range(20 * 16))
    runs = {"validate": lambda: validate(model, ds, ei, 16, scaler=(20.0, 8.0), order=order),
            "evaluate_split": lambda: E.evaluate_split(model, ds, ei, 16, scaler=(20.0, 8.0), order=order)}
    times = {k: [] for k in runs}
    for p in range(1 + a.passes):
        for k, fn in runs.items():
            s = wall(fn)
            if p:
                times[k].append(s)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    say(f"20 batches at B = 16, L_in = 48, fp32: validate {med['validate']:.3f} s, evaluate_split (model + historical average) "
        f"{med['evaluate_split']:.3f} s, ratio {med['evaluate_split'] / med['validate']:.3f}  (all passes: {times})")
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, mean_baseline=rows, split_vs_validate=dict(batches=20, B=16, L_in=48, median_s=med,
                                                                                   all_s=times)), f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
