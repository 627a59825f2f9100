"""Times of the forecast combination (tecmollm/combine.py, csrc/combine.hip) at the shapes it is used at.  Recorded, not
gated: there is no earlier device path to compare with, and no time was promised.

  * the three kernels at B = 16, H = 12, N = 2911, M = 4 (the model's permuted view, the window mean, persistence and a
    node-contiguous forecast as members): device events around back-to-back calls of CombinationMoments.update (one
    tecm_combine_moments launch), CombinationMoments.fit (tecm_combine_solve and the copies of the coefficients to the host)
    and Combination.combine (one tecm_combine_apply launch), with the bytes each call moves;
  * evaluate_split over the same 20 batches at B = 16, L_in = 48 with and without a fitted combination of ("model", "mean",
    "last") in `baselines=`: the median of 3 alternating passes, first pass dropped.

    python tools/combine_bench.py [--out PREFIX] [--no-model]       # writes PREFIX.json and PREFIX.txt
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

from sarima_bench import event_time, split  # noqa: E402  (the TEC-like split of the SARIMA measurements)

T_TEST, H, W, CH, L_OUT = 2208, 41, 71, 6, 12
N = H * W
B, M = 16, 4


def wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combine"))
    ap.add_argument("--no-model", action="store_true", help="skip the evaluate_split comparison (not measured)")
    a = ap.parse_args()
    import torch
    from tecmollm.combine import CombinationMoments, fit_combination, moment_count
    if not torch.cuda.is_available():
        raise SystemExit("combine_bench.py measures on the GPU; none found")
    dev_name = torch.cuda.get_device_name(0)
    lines, rec = [f"# {dev_name}; B = {B}, H = L_out = {L_OUT}, N = {N}, M = {M} members"], {}

    def say(s):
        lines.append(s)
        print(s, flush=True)
    g = torch.Generator(device="cuda").manual_seed(5)
    rand = lambda *shape: torch.randn(*shape, device="cuda", generator=g)
    y = rand(B, L_OUT, N)
    names = ["model", "mean", "last", "linear"]
    preds = [rand(B, N, L_OUT).permute(0, 2, 1) * 0.5 + y, rand(B, 1, N).expand(B, L_OUT, N), rand(B, 1, N).expand(B, L_OUT, N),
             rand(B, L_OUT, N) * 0.3 + y]
    cm = CombinationMoments(names, L_OUT, N)
    K = moment_count(M)
    operand_bytes = (3 * B * L_OUT * N + 2 * B * N) * 4
    stats_bytes = 2 * L_OUT * K * N * 8
    us, n = event_time(torch, lambda: cm.update(preds, y))
    rec["moments"] = dict(call_us_events=us, event_calls=n, operand_bytes=operand_bytes, stats_bytes=stats_bytes, K=K)
    say(f"tecm_combine_moments (device events, {n} back-to-back CombinationMoments.update calls): {us:.1f} us for "
        f"{operand_bytes / 1e6:.1f} MB of operands and {stats_bytes / 1e6:.1f} MB of statistics read and written "
        f"(K = {K}): {(operand_bytes + stats_bytes) / us / 1e3:.0f} GB/s")
    cm.reset()
    for _ in range(8):
        cm.update(preds, y)
    us, n = event_time(torch, lambda: cm.fit(ridge=0.01))
    rec["solve"] = dict(call_us_events=us, event_calls=n, cells=L_OUT * N)
    say(f"CombinationMoments.fit = tecm_combine_solve on {L_OUT * N} cells + coefficients to the host ({n} calls): {us:.1f} us")
    comb = cm.fit(ridge=0.01)
    out = torch.empty(B, L_OUT, N, device="cuda")
    pd = dict(zip(names, preds))
    comb.combine(pd, out=out)
    us, n = event_time(torch, lambda: comb.combine(pd, out=out))
    apply_bytes = operand_bytes - B * L_OUT * N * 4 + B * L_OUT * N * 4 + L_OUT * (M + 1) * N * 8
    rec["apply"] = dict(call_us_events=us, event_calls=n, bytes=apply_bytes)
    say(f"tecm_combine_apply (device events, {n} back-to-back Combination.combine calls): {us:.1f} us for {apply_bytes / 1e6:.1f} MB "
        f"of members, coefficients and output: {apply_bytes / us / 1e3:.0f} GB/s")
    if a.no_model:
        say("evaluate_split with and without a combination: not measured (--no-model)")
    else:
        from baseline_bench import dataset
        from oracle import ref_cpu as R
        from src.model.tec_mollm import TEC_MoLLM
        from tecmollm import evaluate as E
        t = np.arange(T_TEST)
        TF = np.stack([t % 12, t % 366, np.zeros(T_TEST), (t // 30) % 4], 1).astype(np.float32)
        ds = dataset(split(T_TEST, 1).reshape(T_TEST, H, W, CH), TF, 48)
        cfg = R.default_config(L_in=48, L_out=L_OUT, num_nodes=N)
        torch.manual_seed(3)
        with torch.device("cuda"):
            model = TEC_MoLLM(dict(cfg, include_wte=False, load_pretrained_gpt2=False)).eval()
        ei = R.grid_graph()[0].cuda()
        order = list(range(20 * B))
        fit_s = wall(torch, lambda: fit_combination(model, ds, ei, B, members=("model", "mean", "last"), ridge=0.01,
                                                    order=list(range(20 * B, 40 * B))))
        blend = fit_combination(model, ds, ei, B, members=("model", "mean", "last"), ridge=0.01, order=list(range(20 * B, 40 * B)))
        runs = {"without": lambda: E.evaluate_split(model, ds, ei, B, scaler=(20.0, 8.0), baselines=("mean", "last"), order=order),
                "with": lambda: E.evaluate_split(model, ds, ei, B, scaler=(20.0, 8.0), baselines=("mean", "last", blend), order=order)}
        times = {k: [] for k in runs}
        for p in range(4):
            for k, fn in runs.items():                                      # alternating, first pass dropped
                s = wall(torch, fn)
                if p:
                    times[k].append(s)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        rec["evaluate_split"] = dict(batches=20, B=B, L_in=48, median_s=med, all_s=times, fit_combination_wall_s=fit_s)
        say(f"fit_combination over 20 batches at B = {B}, L_in = 48, fp32 (first call, wall): {fit_s:.3f} s")
        say(f"evaluate_split, 20 batches at B = {B}, L_in = 48, fp32: model + mean + last {med['without']:.3f} s, + Combination "
            f"{med['with']:.3f} s, ratio {med['with'] / med['without']:.3f}  (all passes: {times})")
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, **rec), f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
