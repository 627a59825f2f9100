"""Times of AnalogBaseline (src/models/baselines.py, csrc/analog.hip) at the shape it is meant for.  Recorded, not gated: the
feature is new, so nothing of this project is the parent; the yardstick is the same search written with torch on the same
device (`unfold` + batched squared distance + `topk`, over node chunks sized to fit memory).

  * workload: N = 2911 nodes, an archive of Ta = 17 520 rows (four years of 2-hour maps), m = 48, K = 16, L_out = 12, slot keys
    (period 12) off and on;
  * search at S = 16 (one batch of evaluate_split): device events around back-to-back tecm_analog_search calls, the achieved
    rate counted as 2 S n_candidates m N flop per call (one subtraction and one fused multiply-add per term: two vector
    instructions) as a fraction of the fp32 vector peak, and the torch route over the same 16 windows;
  * search over a split of 2000 windows in batches of 16: a host clock around the 125 calls, ended by a synchronise;
  * tecm_analog_forecast at S = 16: the mean alone, and the mean with the K members;
  * evaluate_split with and without the analog baseline over the same 20 batches at B = 16, L_in = 48;
  * kernel times: a child run under `rocprofv3 --kernel-trace --stats` started before this process touches the GPU, first
    launch of every kernel dropped.

    python tools/analog_bench.py [--out PREFIX] [--no-profile] [--no-model]       # writes PREFIX.json and PREFIX.txt
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

from sarima_bench import event_time  # noqa: E402

T_ARCH, T_TEST, H, W, CH, L_IN, L_OUT, M, K = 17520, 2208, 41, 71, 6, 48, 12, 48, 16
N = H * W
S_BATCH, S_SPLIT = 16, 2000
PROFILE_LAUNCHES = 10
FP32_VECTOR_PEAK = 157.3e12                                  # FLOP/s: AMD's datasheet figure for the MI355X
TORCH_NODE_CHUNK = 32                                        # 32 x 17 473 x 16 x 48 floats = 1.7 GB per temporary
KERNELS = ("analog_search", "analog_forecast")


def series(torch, T, seed):
    """(T, N) fp32 on the device: a TEC-like series (diurnal shape x slow amplitude + AR(1) noise), generated there."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(T, device="cuda", dtype=torch.float64)[:, None]
    phase = torch.rand(1, N, device="cuda", dtype=torch.float64, generator=g) * 2 * np.pi
    tec = (1.0 + 0.6 * torch.sin(2 * np.pi * t / 12 + phase)) * 20.0 * (1.0 + 0.3 * torch.sin(2 * np.pi * t / 327.0 + phase))
    eps = torch.randn(T, N, device="cuda", dtype=torch.float64, generator=g)
    noise = torch.zeros_like(eps)
    for i in range(1, T):
        noise[i] = 0.7 * noise[i - 1] + eps[i]
    return ((tec + 1.5 * noise - 20.0) / 8.0).float()


class Work:
    def __init__(self):
        import torch
        from src.models.baselines import AnalogBaseline
        self.torch = torch
        arch = series(torch, T_ARCH + L_OUT, 0)
        self.A = arch[:T_ARCH].t().contiguous()                          # (N, Ta) node-major
        self.Y = (arch * 0.9 + 0.1).t().contiguous()                     # the target-scaled series: another affine map
        test = series(torch, T_TEST, 1)
        self.X = torch.randn(T_TEST, N, CH, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
        self.X[:, :, 0] = test
        self.key_arch = (torch.arange(T_ARCH + 1, device="cuda") % 12).int()
        # a fitted baseline without the dataset object the archive came from: `fit` is one transpose
        ab = AnalogBaseline(k=K, match_len=M)
        ab._A_dev, ab._Y_dev = self.A, self.Y
        ab.slot_ = self.key_arch.cpu().numpy()
        ab.n_candidates_, ab.match_len_, ab.H_, ab.num_nodes_, ab.row0_, ab.L_in_ = T_ARCH - M + 1, M, L_OUT, N, 0, L_IN
        self.ab = ab
        self.ncand = T_ARCH - M + 1

    def keys(self, starts, keyed):
        if not keyed:
            return None, None
        return self.key_arch, ((self.torch.as_tensor(starts) + L_IN) % 12).int().cuda()

    def search(self, starts, keyed):
        from src.models.baselines import analog_search
        ka, kq = self.keys(starts, keyed)
        return analog_search(self.A, T_ARCH + L_OUT, self.X, starts, L_IN, L_OUT, M, K, 0, ka, kq)

    def torch_search(self, starts, keyed):
        """The yardstick: per chunk of nodes the (nodes, candidates, S) table of squared distances from an unfolded view of
        the archive, inadmissible candidates set to +inf, `topk` of the smallest K."""
        torch = self.torch
        S = len(starts)
        rows = (torch.as_tensor(starts)[:, None] + L_IN - M + torch.arange(M)[None, :]).cuda()
        Q = self.X[:, :, 0][rows].permute(2, 0, 1).contiguous()           # (N, S, m)
        Wn = self.A.unfold(1, M, 1)[:, :self.ncand]                       # (N, ncand, m) view
        mask = None
        if keyed:
            ka, kq = self.keys(starts, True)
            mask = ka[M:M + self.ncand][None, :] != kq[:, None]           # (S, ncand): True where refused
        dist = torch.empty(N, S, K, device="cuda")
        idx = torch.empty(N, S, K, device="cuda", dtype=torch.int64)
        for n0 in range(0, N, TORCH_NODE_CHUNK):
            n1 = min(n0 + TORCH_NODE_CHUNK, N)
            d = ((Wn[n0:n1, None, :, :] - Q[n0:n1, :, None, :]) ** 2).sum(-1)          # (nodes, S, ncand)
            if mask is not None:
                d.masked_fill_(mask[None], float("inf"))
            dist[n0:n1], idx[n0:n1] = torch.topk(d, K, dim=2, largest=False, sorted=True)
        return idx.permute(1, 0, 2), dist.permute(1, 0, 2)


def kernels_only():
    from src.models.baselines import analog_forecast
    w = Work()
    starts = list(range(S_BATCH))
    for keyed in (False, True):
        for _ in range(1 + PROFILE_LAUNCHES):
            idx, _, count = w.search(starts, keyed)
    for _ in range(1 + PROFILE_LAUNCHES):
        analog_forecast(w.Y, idx, count, M, L_OUT, want_members=True)
    w.torch.cuda.synchronize()


def profile_kernels(timeout=540):
    """{kernel name fragment: [launches, mean us, min us, max us] per distinct launch order} from a rocprofv3 run of `--kernels-only`:
    the search is launched first without and then with keys, PROFILE_LAUNCHES + 1 times each."""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "analog", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, start, end from kernels order by start").fetchall()
    per = {}
    for name, s, e in rows:
        for frag in KERNELS:
            if frag in name:
                per.setdefault(frag, []).append((e - s) / 1e3)
                break
    out = {}
    us = per.get("analog_search", [])
    if len(us) == 2 * (1 + PROFILE_LAUNCHES):
        for label, part in (("analog_search keys off", us[1:1 + PROFILE_LAUNCHES]), ("analog_search keys on", us[2 + PROFILE_LAUNCHES:])):
            out[label] = (len(part), float(np.mean(part)), float(np.min(part)), float(np.max(part)))
    us = per.get("analog_forecast", [])[1:]
    if us:
        out["analog_forecast mean + members"] = (len(us), float(np.mean(us)), float(np.min(us)), float(np.max(us)))
    return out


def wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analog"))
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
    from src.models.baselines import analog_forecast, analog_search_geometry
    if not torch.cuda.is_available():
        raise SystemExit("analog_bench.py measures on the GPU; none found")
    dev_name = torch.cuda.get_device_name(0)
    lines, rec = [f"# {dev_name}; N = {N}, archive Ta = {T_ARCH}, m = {M}, K = {K}, L_out = {L_OUT}, queries from a {T_TEST}-row split with C = {CH}"], {}

    def say(s):
        lines.append(s)
        print(s, flush=True)
    w = Work()
    chunk, tile, ncand = analog_search_geometry(T_ARCH, T_ARCH + L_OUT, T_TEST, N, CH, 0, L_IN, L_OUT, M, K, S_BATCH)
    flop = 2.0 * S_BATCH * ncand * M * N
    say(f"geometry: chunks of {chunk} candidates, {tile} queries per block, {ncand} candidates; one batch of {S_BATCH} windows = "
        f"{flop / 1e9:.1f} Gflop (2 per term), all of it whether keys are on or off (admission is a mask)")
    starts = list(range(S_BATCH))
    rec["search_batch"] = {}
    for keyed in (False, True):
        label = "keys on" if keyed else "keys off"
        us, n = event_time(torch, lambda: w.search(starts, keyed))
        t_us, tn = event_time(torch, lambda: w.torch_search(starts, keyed), min_seconds=1.0)
        idx, dist, count = w.search(starts, keyed)
        t_idx, t_dist = w.torch_search(starts, keyed)
        same_idx = float((idx.long() == t_idx).float().mean())
        rel = float(((dist - t_dist).abs() / t_dist.clamp_min(1e-30)).max())
        rec["search_batch"][label] = dict(S=S_BATCH, call_us_events=us, event_calls=n, flop=flop, tflops=flop / us / 1e6,
                                          fraction_of_fp32_vector_peak=flop / (us * 1e-6) / FP32_VECTOR_PEAK,
                                          torch_call_us_events=t_us, torch_event_calls=tn, torch_over_kernel=t_us / us,
                                          torch_node_chunk=TORCH_NODE_CHUNK, share_of_equal_indices=same_idx, max_rel_dist_difference=rel,
                                          min_count=int(count.min()))
        say(f"search S = {S_BATCH}, {label}: tecm_analog_search (device events, {n} back-to-back calls, outputs allocated per call) "
            f"{us:.0f} us = {flop / us / 1e6:.2f} TFLOP/s = {flop / (us * 1e-6) / FP32_VECTOR_PEAK * 100:.1f} % of the "
            f"{FP32_VECTOR_PEAK / 1e12:.1f} TFLOP/s fp32 vector peak")
        say(f"  torch route (unfold + squared distance + topk, chunks of {TORCH_NODE_CHUNK} nodes; device events, {tn} calls): {t_us:.0f} us = "
            f"{t_us / us:.1f} x the kernel;  indices equal in {same_idx * 100:.2f} % of the places, distances within {rel:.2e} relative")
    rec["search_split"] = {}
    batches = [list(range(b, min(b + S_BATCH, S_SPLIT))) for b in range(0, S_SPLIT, S_BATCH)]
    for keyed in (False, True):
        label = "keys on" if keyed else "keys off"

        def sweep():
            for chunk_starts in batches:
                w.search(chunk_starts, keyed)
        sweep()
        times = sorted(wall(torch, sweep) for _ in range(3))
        total = 2.0 * S_SPLIT * ncand * M * N
        rec["search_split"][label] = dict(windows=S_SPLIT, batches=len(batches), wall_s=times, median_s=times[1], flop=total,
                                          tflops=total / times[1] / 1e12)
        say(f"search over {S_SPLIT} windows in {len(batches)} batches of {S_BATCH}, {label} (host clock, ended by a synchronise; 3 passes): "
            f"median {times[1]:.3f} s = {total / times[1] / 1e12:.2f} TFLOP/s  (all: {[round(t, 3) for t in times]})")
    idx, _, count = w.search(starts, True)
    rec["forecast"] = {}
    for label, kw in (("mean", dict()), ("mean + members", dict(want_members=True))):
        us, n = event_time(torch, lambda: analog_forecast(w.Y, idx, count, M, L_OUT, **kw))
        rec["forecast"][label] = dict(S=S_BATCH, call_us_events=us, event_calls=n)
        say(f"tecm_analog_forecast S = {S_BATCH}, {label} (device events, {n} calls, outputs allocated per call): {us:.1f} us")
    for label, (cnt, us, lo, hi) in sorted(kern.items()):
        extra = f" = {flop / us / 1e6:.2f} TFLOP/s, {flop / (us * 1e-6) / FP32_VECTOR_PEAK * 100:.1f} % of the fp32 vector peak" if "search" in label else ""
        say(f"kernel time, {label} (rocprofv3 kernel trace, {cnt} launches): {us:.1f} us (min {lo:.1f}, max {hi:.1f}){extra}")
    if not kern:
        say(f"kernel times (rocprofv3): not measured, {why}")
    if a.no_model:
        say("evaluate_split with and without the analog baseline: not measured (--no-model)")
    else:
        from src.data.dataset import SlidingWindowSamplerDataset
        from oracle import ref_cpu as R
        from src.model.tec_mollm import TEC_MoLLM
        from tecmollm import evaluate as E
        t = torch.arange(T_TEST)
        TF = torch.stack([t % 12, t % 366, torch.zeros_like(t), (t // 30) % 4], 1).float()
        Y = w.X[:, :, 0:1].expand(T_TEST, N, L_OUT).reshape(T_TEST, H, W, L_OUT)
        ds = SlidingWindowSamplerDataset.from_tensors(w.X.view(T_TEST, H, W, CH), Y, TF, L_IN, L_OUT, device="cuda", mode="test")
        cfg = R.default_config(L_in=L_IN, L_out=L_OUT, num_nodes=N)
        torch.manual_seed(3)
        with torch.device("cuda"):
            model = TEC_MoLLM(dict(cfg, include_wte=False, load_pretrained_gpt2=False)).eval()
        ei = R.grid_graph()[0].cuda()
        order = list(range(20 * 16))
        runs = {"without": lambda: E.evaluate_split(model, ds, ei, 16, scaler=(20.0, 8.0), baselines=("mean",), order=order),
                "with": lambda: E.evaluate_split(model, ds, ei, 16, scaler=(20.0, 8.0), baselines=("mean", w.ab), order=order)}
        times = {k: [] for k in runs}
        for p in range(4):
            for k, fn in runs.items():                                      # alternating, first pass dropped
                s = wall(torch, fn)
                if p:
                    times[k].append(s)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        rec["evaluate_split"] = dict(batches=20, B=16, L_in=L_IN, median_s=med, all_s=times)
        say(f"evaluate_split, 20 batches at B = 16, L_in = {L_IN}, fp32: model + historical average {med['without']:.3f} s, + Analog "
            f"(slot keys) {med['with']:.3f} s, ratio {med['with'] / med['without']:.3f}  (all passes: {times})")
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, **rec, kernels=kern), f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
