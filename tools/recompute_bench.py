"""Peak memory and step time of the activation-recompute levels (tecmollm/memory.py) on the full graph (N = 2911).

For fp32 and bf16 at (L_in = 48, B = 8) and (L_in = 720, B = 2): levels 0 / 1 / 2 forced through TECM_RECOMPUTE, one
warm-up step each, then --steps timed steps of forward + Huber loss + backward, training mode with dropout (the gradients
are handed over as TrainStep hands them over; the optimizer is not part of the step).  Peak = max_memory_allocated during
the step minus memory_allocated before it; `estimate` is memory.estimate for the same configuration.  Also the eval forward
at L_in = 720, B = 2 in grad mode (level 0) and under torch.no_grad().  --long adds the two configurations that do not fit
at level 0, at the automatic level only: an fp32 training step at L_in = 1440, B = 8 and an fp32 no-grad forward at
L_in = 1440, B = 16 (one warm-up and one timed pass each).

    python tools/recompute_bench.py [--steps 3] [--long] [--out PREFIX]      # writes PREFIX.json and PREFIX.txt
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

N = 2911


def make(L_in, B, prec, train, seed=3):
    from oracle import ref_cpu as R
    from src.model.tec_mollm import TEC_MoLLM
    cfg = R.default_config(L_in=L_in, L_out=12, num_nodes=N, c_in=10, d_emb=12)
    torch.manual_seed(seed)
    with torch.device("cuda"):
        model = TEC_MoLLM(dict(cfg, include_wte=False, load_pretrained_gpt2=False, precision=prec))
    model.train(train)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, L_in, N, 10, device="cuda", generator=g)
    y = torch.randn(B, 12, N, 1, device="cuda", generator=g)
    _, tf, _ = R.synthetic_batch(B, L_in, 1, 10, 12, seed=seed)
    tf = tf[:, :, 0, :].contiguous().cuda().unsqueeze(-2).expand(B, L_in, N, 4)
    return cfg, model, x, tf, R.grid_graph()[0].cuda(), y


def step(model, x, tf, ei, y, grad=True):
    """(ms, peak bytes above the pre-step allocation, level the forward ran at)."""
    from tecmollm import ops
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    if grad:
        out = model(x, tf, ei)
        _, dout = ops.huber_fwd_bwd_strided(out.detach(), y, 1.0, 1.0)
        out.backward(dout)
        del out, dout
    else:
        with torch.no_grad():
            out = model(x, tf, ei)
        del out
    e1.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    model.zero_grad(set_to_none=True)
    return e0.elapsed_time(e1), peak, model.recompute_level


def run(model, x, tf, ei, y, steps, grad=True):
    step(model, x, tf, ei, y, grad)
    res = [step(model, x, tf, ei, y, grad) for _ in range(steps)]
    ms = sorted(r[0] for r in res)
    return ms[len(ms) // 2], ms, max(r[1] for r in res), res[-1][2]


def main():
    from tecmollm import memory
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--long", action="store_true")
    ap.add_argument("--skip-levels", action="store_true", help="only the --long configurations")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recompute_bench"))
    a = ap.parse_args()
    rows, lines = [], []

    def emit(row):
        rows.append(row)
        txt = (f"{row['what']:<34} {row['prec']:<5} L_in {row['L_in']:>5} B {row['B']:>2} level {row['level']} "
               f"peak {row['peak_gb']:7.2f} GB (estimate {row['estimate_gb']:7.2f})  {row['ms']:9.1f} ms")
        lines.append(txt)
        print(txt, flush=True)
    dev = torch.cuda.get_device_name(0)
    free, total = torch.cuda.mem_get_info()
    lines.append(f"# {dev}: {total / 1e9:.1f} GB, {free / 1e9:.1f} GB free at start; N = {N}, c_in 10, 3 GPT-2 blocks")
    if not a.skip_levels:
        for prec in ("fp32", "bf16"):
            code = 1 if prec == "bf16" else 0
            for L_in, B in ((48, 8), (720, 2)):
                cfg, model, x, tf, ei, y = make(L_in, B, prec, True)
                base_ms = None
                for lv in (0, 1, 2):
                    os.environ[memory.ENV] = str(lv)
                    med, ms, peak, got = run(model, x, tf, ei, y, a.steps)
                    base_ms = med if lv == 0 else base_ms
                    est = memory.estimate(cfg, B, code, lv, True, True)
                    emit(dict(what="train step (fwd+loss+bwd)", prec=prec, L_in=L_in, B=B, level=got, ms=med, ms_all=ms,
                              ms_ratio_to_level0=med / base_ms, peak_gb=peak / 1e9, estimate_gb=est.peak / 1e9,
                              estimate_kept_gb=est.kept / 1e9))
                del model, x, tf, ei, y
                torch.cuda.empty_cache()
        cfg, model, x, tf, ei, y = make(720, 2, "fp32", False)
        os.environ[memory.ENV] = "0"
        med, ms, peak, got = run(model, x, tf, ei, y, a.steps, grad=False)
        est = memory.estimate(cfg, 2, 0, 0, False, False)
        emit(dict(what="eval forward, no grad", prec="fp32", L_in=720, B=2, level=got, ms=med, ms_all=ms,
                  peak_gb=peak / 1e9, estimate_gb=est.peak / 1e9))
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = model(x, tf, ei)
        torch.cuda.synchronize()
        emit(dict(what="eval forward, grad mode", prec="fp32", L_in=720, B=2, level=model.recompute_level, ms=float("nan"),
                  peak_gb=(torch.cuda.max_memory_allocated() - base) / 1e9,
                  estimate_gb=float("nan")))
        del out, model, x, tf, ei, y
        torch.cuda.empty_cache()
    if a.long:
        os.environ.pop(memory.ENV, None)
        memory.clear_choices()
        for what, L_in, B, train, grad in (("train step, automatic level", 1440, 8, True, True),
                                           ("eval forward, no grad", 1440, 16, False, False)):
            try:
                cfg, model, x, tf, ei, y = make(L_in, B, "fp32", train)
                budget = memory.device_budget(torch.device("cuda"))
                med, ms, peak, got = run(model, x, tf, ei, y, 1, grad=grad)
                est = memory.estimate(cfg, B, 0, got, train, grad)
                e0 = memory.estimate(cfg, B, 0, 0, train, grad)
                emit(dict(what=what, prec="fp32", L_in=L_in, B=B, level=got, ms=med, ms_all=ms, peak_gb=peak / 1e9,
                          estimate_gb=est.peak / 1e9, estimate_level0_gb=e0.peak / 1e9, budget_gb=budget / 1e9))
                del model, x, tf, ei, y
            except torch.cuda.OutOfMemoryError as e:                      # recorded, not retried
                rows.append(dict(what=what, L_in=L_in, B=B, error=str(e)[:300]))
                lines.append(f"{what} L_in {L_in} B {B}: out of memory")
                print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    with open(a.out + ".json", "w") as f:
        json.dump(dict(device=dev, rows=rows), f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
