"""Cost of the raw-data stage at the training split's size, T = 39 420 steps of N = 2911 nodes with Ci = 5 indices (float32
TEC, float64 indices).  Recorded, not gated.

  * kernel times of the moments kernels (the feature fit: TEC pooled over T - 12 rows, the five index columns; the target
    fit: TEC pooled with taps = 12), of features_x_kernel + features_ys_kernel (the series layout of one split) and of
    features_y_kernel (the materialised Y, at T_SMALL = 4380 rows), of the target part of a batch of B = 16 windows by
    `tecm_window_batch_series` (window_x_kernel over Ys) and by today's window_y_kernel on a materialised Y of T_SMALL rows:
    a run of its own under `rocprofv3 --kernel-trace --stats` (a child process started before this one touches the GPU),
    read from the trace database, first launch of every case dropped;
  * algorithmic bytes (every input read once per pass, every output written once) and the fraction of 6.3 TB/s;
  * wall time of `preprocess_splits` end to end from host arrays (train 39 420, val 8760, test 5832 rows; upload, both fits,
    every split built, one device synchronise), and at T_SMALL = 4380 rows (one year as the training split, val and test
    of 1200 rows) next to the numpy / sklearn path on the host at that size: X and the 12-fold Y built in float64,
    `StandardScaler().fit` on both, transform, cast to float32;
  * resident bytes of a series-backed split against a materialised one.

    python tools/preprocess_bench.py [--out PREFIX] [--no-profile] [--no-host]      # writes PREFIX.json and PREFIX.txt
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

T, H, W, CI, HORIZON = 39420, 41, 71, 5, 12
N = H * W
T_SMALL = 4380
ROWS = {"train": T, "val": 8760, "test": 5832}
B, L_IN = 16, 48
PROFILE_LAUNCHES = 5
HBM_BYTES_PER_S = 6.3e12


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def raw_split(rows, seed, start="2013-01-01T00"):
    rng = np.random.default_rng(seed)
    tec = rng.standard_gamma(2.0, size=(rows, H, W), dtype=np.float32) * np.float32(12.0)
    idx = rng.normal(50.0, 20.0, size=(rows, CI))
    time_ = np.datetime64(start, "s") + 7200 * np.arange(rows).astype("timedelta64[s]")
    return {"tec": tec, "space_weather_indices": idx, "time": time_}


def kernels_only():
    """The child run under the profiler: per case one warm-up call and PROFILE_LAUNCHES more."""
    import torch
    from src.data.dataset import SeriesWindowDataset, SlidingWindowSamplerDataset
    from tecmollm.preprocess import DeviceStandardScaler, build_features, moments
    raw = raw_split(T, 0)
    tec = torch.from_numpy(raw["tec"]).cuda().reshape(T, N)
    idx = torch.from_numpy(raw["space_weather_indices"]).cuda()
    per = 1 + PROFILE_LAUNCHES
    for _ in range(per):
        moments(tec[:T - HORIZON], pool=True)
    for _ in range(per):
        moments(idx[:T - HORIZON], pool=False)
    for _ in range(per):
        moments(tec, pool=True, taps=HORIZON)
    torch.cuda.synchronize()
    fs = DeviceStandardScaler(np.full(6, 20.0), None, np.full(6, 15.0))
    ts = DeviceStandardScaler([24.0], None, [17.0])
    for _ in range(per):
        out = build_features(tec, idx, fs, ts, outputs=("X", "Ys"))
        torch.cuda.synchronize()
    for _ in range(per):
        y = build_features(tec[:T_SMALL], None, None, ts, horizon=HORIZON, outputs=("Y",))["Y"]
        torch.cuda.synchronize()
    tf = torch.zeros(T_SMALL, 4, device="cuda")
    X = out["X"][:T_SMALL].reshape(T_SMALL, H, W, 1 + CI)
    new = SeriesWindowDataset.from_series(X, out["Ys"][:T_SMALL].reshape(T_SMALL, H, W), tf, L_IN, HORIZON)
    old = SlidingWindowSamplerDataset.from_tensors(X[:T_SMALL - HORIZON], y.reshape(T_SMALL - HORIZON, H, W, HORIZON),
                                                   tf[:T_SMALL - HORIZON], L_IN, HORIZON)
    starts = [int(i) for i in np.random.default_rng(1).integers(0, len(old), B)]
    for ds in (new, old):
        for _ in range(per):
            ds.batch(starts)
        torch.cuda.synchronize()


def profile_kernels(timeout=900):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "preprocess", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, start, end from kernels order by start").fetchall()
    per = 1 + PROFILE_LAUNCHES
    # the trace holds mangled or demangled names, depending on the profiler's version: `any2` lists both spellings of a pass
    us = lambda frag, any2=("",): [(e - s) / 1e3 for name, s, e in rows if frag in name and any(f in name for f in any2)]
    p0, p1 = ("Li0E", ", 0>", ",0>"), ("Li1E", ", 1>", ",1>")
    summary = lambda u: (len(u), float(np.mean(u)), float(np.min(u)), float(np.max(u)))
    pool0, pool1 = us("moments_pool_kernel", p0), us("moments_pool_kernel", p1)
    col0, col1 = us("moments_col_kernel", p0), us("moments_col_kernel", p1)
    join = us("moments_join_kernel")
    fx, fys, fy = us("features_x_kernel"), us("features_ys_kernel"), us("features_y_kernel")
    wx, wy = us("window_x_kernel"), us("window_y_kernel")
    want = dict(pool0=2 * per, pool1=2 * per, col0=per, col1=per, join=6 * per, fx=per, fys=per, fy=per, wx=3 * per, wy=per)
    have = dict(pool0=len(pool0), pool1=len(pool1), col0=len(col0), col1=len(col1), join=len(join), fx=len(fx), fys=len(fys),
                fy=len(fy), wx=len(wx), wy=len(wy))
    if have != want:
        raise RuntimeError(f"unexpected launch counts: {have}, expected {want}")
    series_y = wx[1:2 * per:2]                                             # the series batches launch window_x twice: x, then y
    return {
        "moments_pool_kernel<float, sum> feature fit": summary(pool0[1:per]),
        "moments_pool_kernel<float, squares> feature fit": summary(pool1[1:per]),
        "moments_pool_kernel<float, sum> target fit, taps 12": summary(pool0[per + 1:]),
        "moments_pool_kernel<float, squares> target fit, taps 12": summary(pool1[per + 1:]),
        "moments_col_kernel<double, sum> 5 index columns": summary(col0[1:]),
        "moments_col_kernel<double, squares> 5 index columns": summary(col1[1:]),
        "moments_join_kernel": summary(join[6:]),
        "features_x_kernel": summary(fx[1:]),
        "features_ys_kernel": summary(fys[1:]),
        "features_y_kernel": summary(fy[1:]),
        "window_x_kernel over Ys (tecm_window_batch_series target)": summary(series_y[1:]),
        "window_y_kernel (tecm_window_batch target)": summary(wy[1:]),
    }


def algorithmic_bytes():
    fit_rows = T - HORIZON
    batch = 2 * B * HORIZON * N * 4
    return {
        "moments_pool_kernel<float, sum> feature fit": fit_rows * N * 4,
        "moments_pool_kernel<float, squares> feature fit": fit_rows * N * 4,
        "moments_pool_kernel<float, sum> target fit, taps 12": T * N * 4,
        "moments_pool_kernel<float, squares> target fit, taps 12": T * N * 4,
        "moments_col_kernel<double, sum> 5 index columns": fit_rows * CI * 8,
        "moments_col_kernel<double, squares> 5 index columns": fit_rows * CI * 8,
        "moments_join_kernel": 2048 * 16,
        "features_x_kernel": T * N * 4 + T * CI * 8 + T * N * (1 + CI) * 4,
        "features_ys_kernel": 2 * T * N * 4,
        "features_y_kernel": T_SMALL * N * 4 + (T_SMALL - HORIZON) * N * HORIZON * 4,
        "window_x_kernel over Ys (tecm_window_batch_series target)": batch,
        "window_y_kernel (tecm_window_batch target)": batch,
    }


def host_path(splits):
    """The numpy / sklearn path: X and the horizon-fold Y in float64, both scalers fitted on the training split, every split
    transformed and cast to float32."""
    from sklearn.preprocessing import StandardScaler
    built = {}
    for name, d in splits.items():
        tec = d["tec"]
        rows = tec.shape[0] - HORIZON
        idx = np.broadcast_to(d["space_weather_indices"][:rows, None, None, :], (rows, H, W, CI))
        X = np.concatenate([tec[:rows, :, :, None].astype(np.float64), idx], axis=-1)
        Y = np.zeros((rows, H, W, HORIZON))
        for i in range(rows):
            Y[i] = tec[i + 1:i + 1 + HORIZON].transpose(1, 2, 0)
        built[name] = (X, Y)
    fs = StandardScaler().fit(built["train"][0].reshape(-1, 1 + CI))
    ts = StandardScaler().fit(built["train"][1].reshape(-1, 1))
    return {name: (fs.transform(X.reshape(-1, 1 + CI)).reshape(X.shape).astype(np.float32),
                   ts.transform(Y.reshape(-1, 1)).reshape(Y.shape).astype(np.float32)) for name, (X, Y) in built.items()}, fs, ts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (kernel time: not measured)")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy / sklearn path on the host")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    kern = {} if a.no_profile else profile_kernels()                       # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench.py measures on the GPU; none found")
    from tecmollm import preprocess_splits
    dev_name = torch.cuda.get_device_name(0)
    lines, rows = [f"# {dev_name}; T = {T}, N = {N}, Ci = {CI}, horizon {HORIZON}, float32 TEC, float64 indices; "
                   f"python tools/preprocess_bench.py" + (" --no-profile" if a.no_profile else "") + f" --passes {a.passes}"], []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    nbytes = algorithmic_bytes()
    for name, (cnt, us, lo, hi) in kern.items():
        frac = nbytes[name] / (us * 1e-6) / HBM_BYTES_PER_S
        rows.append(dict(kernel=name, algorithmic_bytes=nbytes[name], kernel_us=us, kernel_us_min=lo, kernel_us_max=hi, launches=cnt,
                         algorithmic_GBps=nbytes[name] / us / 1e3, fraction_of_6p3_TBps=frac))
        say(f"{name}: {us:.1f} us (min {lo:.1f}, max {hi:.1f}; rocprofv3 kernel trace, {cnt} launches), algorithmic "
            f"{nbytes[name] / 1e6:.2f} MB -> {nbytes[name] / us / 1e3:.0f} GB/s = {100 * frac:.1f} % of 6.3 TB/s")
    if not kern:
        say("kernel time: not measured")
    # ---- end to end at the full size, from host arrays
    full = {name: raw_split(r, seed) for seed, (name, r) in enumerate(ROWS.items())}
    times, res = [], {}
    for p in range(1 + a.passes):
        res.clear()
        s = wall(lambda: res.update(out=preprocess_splits(full, horizon=HORIZON)))
        if p:
            times.append(s)
    out = res["out"]
    say(f"preprocess_splits end to end, rows {ROWS}, from host arrays to the series layout on the device: median "
        f"{sorted(times)[len(times) // 2]:.3f} s of {times} (host clock around a synchronise; upload, both fits, every split built)")
    tr = out["train"]
    series_b = sum(tr[k].numel() * tr[k].element_size() for k in ("X", "Ys", "time_features"))
    rows_m = T - HORIZON
    mat_b = rows_m * N * (1 + CI) * 4 + rows_m * N * HORIZON * 4 + rows_m * 4 * 4
    say(f"resident bytes of the training split: series-backed X + Ys + time features {series_b / 1e9:.3f} GB, materialised "
        f"X + Y (horizon {HORIZON}) + time features {mat_b / 1e9:.3f} GB ({mat_b / series_b:.2f} x); horizon 24 materialised: "
        f"{((T - 24) * N * ((1 + CI) + 24) * 4 + (T - 24) * 16) / 1e9:.3f} GB")
    del out, tr, full
    res.clear()
    torch.cuda.empty_cache()
    # ---- one year, next to the host path
    small = {"train": raw_split(T_SMALL, 10), "val": raw_split(1200, 11), "test": raw_split(1200, 12)}
    dev_times = []
    for p in range(1 + a.passes):
        s = wall(lambda: res.update(out=preprocess_splits(small, horizon=HORIZON, layout="reference")))
        if p:
            dev_times.append(s)
    dev_med = sorted(dev_times)[len(dev_times) // 2]
    host = {}
    if not a.no_host:
        t0 = time.perf_counter()
        built, fs, ts = host_path(small)
        host["seconds"] = time.perf_counter() - t0
        got = res["out"]
        host["identical_X"] = bool(all(np.array_equal(got[k]["X"].cpu().numpy(), built[k][0]) for k in built))
        host["identical_Y"] = bool(all(np.array_equal(got[k]["Y"].cpu().numpy(), built[k][1]) for k in built))
        host["max_ulp_note"] = "the fits differ in the last bits (different summation order), so values may differ by one float32 step"
        host["scaler_mean_rel_diff"] = float(abs(got.target_scaler.mean_[0] - ts.mean_[0]) / abs(ts.mean_[0]))
        say(f"T = {T_SMALL} (train) + 1200 + 1200 rows, reference layout: preprocess_splits {dev_med:.3f} s (median of {dev_times}); "
            f"numpy / sklearn on the host (X and the {HORIZON}-fold Y in float64, {os.cpu_count()} CPUs visible, the host path was "
            f"run at this size only) {host['seconds']:.1f} s; identical X: {host['identical_X']}, identical Y: {host['identical_Y']}; "
            f"target mean relative difference {host['scaler_mean_rel_diff']:.2e}")
    else:
        say(f"T = {T_SMALL} (train) + 1200 + 1200 rows, reference layout: preprocess_splits {dev_med:.3f} s (median of {dev_times}); "
            "host path: not measured")
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, T=T, N=N, Ci=CI, horizon=HORIZON, T_small=T_SMALL, rows=ROWS, kernel=rows,
                       wall=dict(full_s=times, small_device_s=dev_times, small_host=host),
                       resident=dict(series_bytes=series_b, materialised_bytes=mat_b)), f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
