"""Cost of the quantile path at the full grid, N = 2911, L_out = 12, B = 8, Q = 3 levels.  Recorded, not gated.

  * the pinball kernel pair (tecm_pinball_fwd_bwd_strided, loss + per-level losses + gradient on the head's permuted
    (B, Q * L_out, N, 1) view) next to the Huber pair (tecm_huber_fwd_bwd_strided on a (B, L_out, N, 1) view): device
    events around LAUNCHES back-to-back calls (allocations of the wrappers included on both sides), per call;
  * one `QuantileMetrics.update` (tecm_quantile_stats) per batch, the levels read in place from the model's layout, with
    and without a CQR adjust, the same way;
  * a training step (`TrainStep.step`, forward + loss + backward + clip + AdamW, fp32, L_in = 48, training mode) of the
    Q = 3 model with the pinball loss next to the Q = 1 model with the Huber loss in the same run (the head and its gradient
    are 3x wider): host clock around a synchronise, median of `--passes` alternating passes after one warm-up pass.

    python tools/quantile_bench.py [--out PREFIX] [--passes P]             # writes PREFIX.json and PREFIX.txt
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tec-mollm_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from baseline_bench import L_OUT, N, wall  # noqa: E402

B = 8
L_IN = 48
TAUS = (0.1, 0.5, 0.9)
LAUNCHES = 50
SCALER = (20.0, 8.0)


def per_call_us(fn, passes):
    """Median over `passes` of (device time of LAUNCHES calls) / LAUNCHES, after one warm-up pass; microseconds."""
    import torch
    out = []
    for p in range(1 + passes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if p:
            out.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    return sorted(out)[len(out) // 2], out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile"))
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("quantile_bench.py measures on the GPU; none found")
    from oracle import ref_cpu as R
    from src.evaluation.metrics import QuantileMetrics
    from src.model.tec_mollm import TEC_MoLLM
    from tecmollm import PinballLoss, ops, quantile_config
    from tecmollm.functions import quantile_view
    from tecmollm.train import TrainStep
    dev_name = torch.cuda.get_device_name(0)
    Q = len(TAUS)
    lines, rec = [f"# {dev_name}; N = {N}, L_out = {L_OUT}, B = {B}, Q = {Q}; python tools/quantile_bench.py --passes {a.passes}"], {}

    def say(s):
        lines.append(s)
        print(s, flush=True)
    torch.manual_seed(0)
    y = torch.randn(B, L_OUT, N, 1, device="cuda")
    out1 = torch.randn(B, N, L_OUT, device="cuda").permute(0, 2, 1).unsqueeze(-1)
    outq = torch.randn(B, N, Q * L_OUT, device="cuda").permute(0, 2, 1).unsqueeze(-1)
    lv = quantile_view(outq, Q)
    hub, hub_all = per_call_us(lambda: ops.huber_fwd_bwd_strided(out1, y, 1.0, 1.0), a.passes)
    pin, pin_all = per_call_us(lambda: ops.pinball_fwd_bwd_strided(lv, y, TAUS, 1.0), a.passes)
    rec["loss_pair_us"] = dict(huber=hub, pinball=pin, huber_all=hub_all, pinball_all=pin_all, launches=LAUNCHES)
    say(f"loss + gradient, two kernels per call: Huber (B, {L_OUT}, N) {hub:.1f} us, pinball (B, {Q}, {L_OUT}, N) {pin:.1f} us "
        f"per call ({Q}x the elements; device events around {LAUNCHES} calls, median of {a.passes} passes)")
    qm = QuantileMetrics(L_OUT, N, TAUS, 1, SCALER)
    adj = torch.zeros(1, L_OUT, Q, N, device="cuda")
    st, st_all = per_call_us(lambda: qm.update(lv, y), a.passes)
    sa, sa_all = per_call_us(lambda: qm.update(lv, y, None, adj), a.passes)
    nbytes = (Q + 1) * B * L_OUT * N * 4 + 2 * L_OUT * N * (1 + Q + Q // 2) * 12
    rec["quantile_stats_us"] = dict(plain=st, adjust=sa, plain_all=st_all, adjust_all=sa_all, algorithmic_bytes=nbytes)
    say(f"QuantileMetrics.update (tecm_quantile_stats), one batch: {st:.1f} us, with a CQR adjust {sa:.1f} us per call; "
        f"algorithmic {nbytes / 1e6:.2f} MB -> {nbytes / st / 1e3:.0f} GB/s")
    # the training step, Q = 3 with the pinball loss against Q = 1 with the Huber loss
    base = R.default_config(L_in=L_IN, L_out=L_OUT, num_nodes=N)
    x, tf, _ = R.synthetic_batch(B, L_IN, N, base["spatial_in_channels_base"], L_OUT, seed=1)
    x = x.cuda()
    tf = tf[:, :, 0, :].contiguous().cuda().unsqueeze(-2).expand(B, L_IN, N, 4)
    ei = R.grid_graph()[0].cuda()
    steps = {}
    for name, cfg, loss in (("Q=1 huber", base, "huber"), (f"Q={Q} pinball", quantile_config(base, TAUS), PinballLoss(TAUS))):
        torch.manual_seed(3)
        with torch.device("cuda"):
            model = TEC_MoLLM(dict(cfg, include_wte=False, load_pretrained_gpt2=False)).train()
        ts = TrainStep(model, loss=loss)
        steps[name] = lambda ts=ts: ts.step(x, tf, ei, None, y)
    times = {k: [] for k in steps}
    for p in range(1 + a.passes):
        for k, fn in steps.items():
            s = wall(fn)
            if p:
                times[k].append(s)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    k1, kq = list(steps)
    rec["train_step_s"] = dict(median=med, all=times, B=B, L_in=L_IN)
    say(f"TrainStep.step, B = {B}, L_in = {L_IN}, fp32, training mode: {k1} {med[k1] * 1e3:.1f} ms, {kq} {med[kq] * 1e3:.1f} ms "
        f"(x{med[kq] / med[k1]:.3f}; host clock around a synchronise, median of {a.passes} alternating passes)")
    say(f"all passes, seconds: {times}")
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev_name, **rec), f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
