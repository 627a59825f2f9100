"""Times of LinearBaseline (src/models/baselines.py, csrc/linear.hip) at the shapes it is used at.  Recorded, not gated: there
is no earlier device path to compare with, and no time was promised.

  * fit: the full training split, T = 4380 two-hourly steps, N = 2911, C = 6, the default 48 look-backs of channel 0 and the
    intercept (P = 49), H = 12, every stride-1 window: device events around back-to-back tecm_lin_gram and tecm_lin_solve
    calls, the wall time of LinearBaseline.fit_series (+ the copies of the results), and the Gram kernel's fp64 FMA rate as a
    fraction of the fp64 vector peak (78.6 TFLOP/s: AMD's datasheet figure, half the fp32 vector rate);
  * forecast: every stride-1 window of a full test split (T = 2208), L_in = 48 and 336, L_out = 12, one tecm_lin_forecast
    launch into a (windows, 12, N) buffer, beside SARIMA's forecast and the window mean over the same windows in the same run;
  * evaluate_split with and without the linear baseline over the same 20 batches at B = 16, L_in = 48;
  * kernel times: a child run under `rocprofv3 --kernel-trace --stats` started before this process touches the GPU, first
    launch of every kernel dropped.

    python tools/linear_bench.py [--out PREFIX] [--no-profile] [--no-model]       # writes PREFIX.json and PREFIX.txt
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

from sarima_bench import event_time, split  # noqa: E402  (the TEC-like split of the SARIMA measurements)

T_TRAIN, T_TEST, H, W, CH, L_OUT = 4380, 2208, 41, 71, 6, 12
N = H * W
CASES = (48, 336)
FIT_L_IN = 48
PROFILE_LAUNCHES = 10
FP64_VECTOR_PEAK = 78.6e12                                   # FLOP/s
KERNELS = ("lin_gram", "lin_pool", "lin_solve", "lin_forecast")


class Work:
    def __init__(self):
        import torch
        from src.models.baselines import LinearBaseline, SarimaBaseline, linear_pairs
        self.torch = torch
        self.train = torch.from_numpy(split(T_TRAIN, 0)).cuda()
        self.test = torch.from_numpy(split(T_TEST, 1)).cuda()
        # the target-scaled series: channel 0 under another affine map, a tensor of its own as in a series file
        self.ys = (self.train[:, :, 0] * 0.05 - 1.0).contiguous()
        self.pairs = linear_pairs(None, 0, (), FIT_L_IN)
        self.count = T_TRAIN - FIT_L_IN - L_OUT + 1
        self.lb = LinearBaseline()
        self.sb = SarimaBaseline()

    def gram(self):
        from src.models.baselines import linear_gram
        return linear_gram(self.train, self.ys, self.pairs, FIT_L_IN, L_OUT, 0, 1, self.count)[0]

    def fit(self):
        return self.lb.fit_series(self.train, self.ys, FIT_L_IN, L_OUT, 0, 1, self.count)

    def forecaster(self, model, L_in):
        S = T_TEST - L_in - L_OUT + 1
        starts = list(range(S))
        out = self.torch.empty(S, L_OUT, N, device="cuda")
        coef = model._coef_on(self.test.device)
        return S, lambda: model.forecast_series(self.test, starts, L_in, L_OUT, out=out, coef=coef)

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
    from src.models.baselines import linear_solve
    w = Work()
    for _ in range(1 + PROFILE_LAUNCHES):
        linear_solve(w.gram(), 1.0)
    w.fit()
    for L_in in CASES:
        _, run = w.forecaster(w.lb, L_in)
        for _ in range(1 + PROFILE_LAUNCHES):
            run()
    w.torch.cuda.synchronize()


def profile_kernels(timeout=540):
    """{kernel name fragment: {grid blocks: (launches, mean us, min us, max us)}} from a rocprofv3 run of `--kernels-only`."""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "linear", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, grid_x, workgroup_x, start, end from kernels order by start").fetchall()
    per = {}
    for name, gx, wx, s, e in rows:
        for frag in KERNELS:
            if frag in name:
                per.setdefault(frag, {}).setdefault(gx // wx, []).append((e - s) / 1e3)
                break
    return {f: {b: (len(us) - 1, float(np.mean(us[1:])), float(np.min(us[1:])), float(np.max(us[1:])))
                for b, us in by.items() if len(us) > 1} for f, by in per.items()}


def wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (kernel times: not measured)")
    ap.add_argument("--no-model", action="store_true", help="skip the evaluate_split comparison (not measured)")
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
    from src.models.baselines import linear_gram_geometry, linear_solve
    if not torch.cuda.is_available():
        raise SystemExit("linear_bench.py measures on the GPU; none found")
    dev_name = torch.cuda.get_device_name(0)
    lines, rec = [f"# {dev_name}; N = {N}, C = {CH}, lags 1..48 of channel 0 + intercept (P = 49), H = L_out = {L_OUT}, stride 1"], {}

    def say(s):
        lines.append(s)
        print(s, flush=True)
    w = Work()
    P, count = len(w.pairs) + 1, w.count
    tile, chunk = linear_gram_geometry(w.pairs, T_TRAIN, N, CH, T_TRAIN, FIT_L_IN, L_OUT, 0, 1, count)
    useful = count * N * P * (P + L_OUT)
    issued = count * (-(-N // tile) * tile) * (-(-P // 8) * 8) * (-(-(P + L_OUT) // 4) * 4)
    gram_us, n = event_time(torch, w.gram)
    g = w.gram()
    solve_us, n2 = event_time(torch, lambda: linear_solve(g, 1.0))
    walls = sorted(wall(torch, w.fit) for _ in range(3))
    st = w.lb.status_
    rec["fit"] = dict(T=T_TRAIN, windows=count, P=P, H=L_OUT, tile_nodes=tile, chunk_windows=chunk, useful_fma=useful,
                      issued_fma=issued, gram_call_us_events=gram_us, gram_event_calls=n, solve_call_us_events=solve_us,
                      solve_event_calls=n2, fit_series_wall_s=walls[1], degenerate=int((st & 1 != 0).sum()),
                      nonfinite=int((st & 2 != 0).sum()),
                      gram_useful_fraction_of_fp64_peak=2 * useful / (gram_us * 1e-6) / FP64_VECTOR_PEAK,
                      gram_issued_fraction_of_fp64_peak=2 * issued / (gram_us * 1e-6) / FP64_VECTOR_PEAK)
    say(f"fit, training split T = {T_TRAIN}: {count} windows x {N} nodes, [G | R] {P} x {P + L_OUT}: {useful / 1e9:.2f} G useful fp64 FMAs, "
        f"{issued / 1e9:.2f} G issued (8 x 4 lane rectangles, tiles of {tile} nodes); chunks of {chunk} windows")
    say(f"  tecm_lin_gram (device events, {n} back-to-back calls, allocation of the output included): {gram_us:.1f} us = "
        f"{2 * useful / gram_us / 1e6:.2f} TFLOP/s useful = {rec['fit']['gram_useful_fraction_of_fp64_peak'] * 100:.1f} % of the "
        f"{FP64_VECTOR_PEAK / 1e12:.1f} TFLOP/s fp64 vector peak ({rec['fit']['gram_issued_fraction_of_fp64_peak'] * 100:.1f} % counting the padded lanes)")
    say(f"  tecm_lin_solve, {N} systems of {P} x {P} with {L_OUT} right-hand sides (device events, {n2} calls): {solve_us:.1f} us")
    say(f"  LinearBaseline.fit_series wall (+ results and the last window to the host): {walls[1] * 1e3:.1f} ms;  status: "
        f"{rec['fit']['degenerate']} degenerate, {rec['fit']['nonfinite']} non-finite of {N}")
    for frag in ("lin_gram", "lin_solve"):
        for blocks, (cnt, us, lo, hi) in sorted(kern.get(frag, {}).items()):
            say(f"    {frag}_kernel ({blocks} blocks; rocprofv3 kernel trace, {cnt} launches): {us:.1f} us (min {lo:.1f}, max {hi:.1f})")
            if frag == "lin_gram":
                rec["fit"].update(gram_kernel_us=us, gram_kernel_useful_fraction_of_fp64_peak=2 * useful / (us * 1e-6) / FP64_VECTOR_PEAK)
                say(f"      = {2 * useful / us / 1e6:.2f} TFLOP/s useful, {2 * useful / (us * 1e-6) / FP64_VECTOR_PEAK * 100:.1f} % of the fp64 vector peak")
    w.sb.fit(w.train[:, :, 0])
    rec["forecast"] = []
    for L_in in CASES:
        S, run = w.forecaster(w.lb, L_in)
        us, n = event_time(torch, run)
        sar_us, _ = event_time(torch, w.forecaster(w.sb, L_in)[1])
        mean_us, _ = event_time(torch, w.mean_launch(L_in))
        read = S * (P - 1) * N * 4
        row = dict(L_in=L_in, windows=S, call_us_events=us, event_calls=n, sarima_call_us_events=sar_us,
                   window_mean_call_us_events=mean_us, predictor_bytes=read, output_bytes=S * L_OUT * N * 4)
        say(f"forecast L_in {L_in:>3}: {S} windows x {N} nodes, {read / 1e9:.3f} GB of predictor values, {S * L_OUT * N * 4 / 1e6:.0f} MB written")
        say(f"  tecm_lin_forecast (device events, {n} back-to-back launches): {us:.1f} us;  tecm_sar_forecast over the same windows, "
            f"same method: {sar_us:.1f} us;  tecm_window_baseline MEAN: {mean_us:.1f} us")
        for blocks, (cnt, kus, lo, hi) in sorted(kern.get("lin_forecast", {}).items()):
            if blocks == -(-(-(-S // 4)) // 4) * ((N + 63) // 64):          # 4 windows per thread, 4 such groups per block
                row.update(kernel_us=kus, kernel_us_min=lo, kernel_us_max=hi)
                say(f"  kernel time (rocprofv3 kernel trace, {cnt} launches): {kus:.1f} us (min {lo:.1f}, max {hi:.1f})")
        rec["forecast"].append(row)
    if not kern:
        say(f"kernel times (rocprofv3): not measured, {why}")
    if a.no_model:
        say("evaluate_split with and without the linear baseline: not measured (--no-model)")
    else:
        from baseline_bench import dataset
        from oracle import ref_cpu as R
        from src.model.tec_mollm import TEC_MoLLM
        from tecmollm import evaluate as E
        t = np.arange(T_TEST)
        TF = np.stack([t % 12, t % 366, np.zeros(T_TEST), (t // 30) % 4], 1).astype(np.float32)
        ds = dataset(w.test.cpu().numpy().reshape(T_TEST, H, W, CH), TF, 48)
        cfg = R.default_config(L_in=48, L_out=L_OUT, num_nodes=N)
        torch.manual_seed(3)
        with torch.device("cuda"):
            model = TEC_MoLLM(dict(cfg, include_wte=False, load_pretrained_gpt2=False)).eval()
        ei = R.grid_graph()[0].cuda()
        order = list(range(20 * 16))
        runs = {"without": lambda: E.evaluate_split(model, ds, ei, 16, scaler=(20.0, 8.0), baselines=("mean",), order=order),
                "with": lambda: E.evaluate_split(model, ds, ei, 16, scaler=(20.0, 8.0), baselines=("mean", w.lb), order=order)}
        times = {k: [] for k in runs}
        for p in range(4):
            for k, fn in runs.items():                                      # alternating, first pass dropped
                s = wall(torch, fn)
                if p:
                    times[k].append(s)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        rec["evaluate_split"] = dict(batches=20, B=16, L_in=48, median_s=med, all_s=times)
        say(f"evaluate_split, 20 batches at B = 16, L_in = 48, fp32: model + historical average {med['without']:.3f} s, + Linear "
            f"{med['with']:.3f} s, ratio {med['with'] / med['without']:.3f}  (all passes: {times})")
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, **rec, kernels={k: {str(b): v for b, v in by.items()} for k, by in kern.items()}), f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
