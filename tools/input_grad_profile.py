#!/usr/bin/env python3
"""Training steps with `x.requires_grad` at the timed size, for a kernel trace of the input gradient next to the parameter
backward of the spatial stage (profiles/input_grad.txt):

    rocprofv3 --kernel-trace --stats -d OUT -o ig -- python tools/input_grad_profile.py [--steps 3]
    python tools/rocpd_stats.py OUT/ig_results.db --skip-first 1 | grep spatial

fp32, B = 8, L_in = 48, N = 2911, every graph with edges, dropout on; one warm-up step, then `--steps` steps.  Prints the
wall time per step with and without `x.requires_grad` (device-synchronised; under the profiler it only orders the two)."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from src.model.tec_mollm import TEC_MoLLM  # noqa: E402
from tecmollm import functions as F_  # noqa: E402
from tecmollm.synthetic import grid_graph, synthetic_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--L_in", type=int, default=48)
    a = ap.parse_args()
    dev = torch.device("cuda")
    cfg = {"num_nodes": 2911, "d_emb": 16, "spatial_in_channels_base": 6, "spatial_out_channels": 11, "spatial_heads": 2,
           "temporal_channel_list": [64, 128], "temporal_strides": [2, 2], "patch_len": 4, "d_llm": 768, "llm_layers": 3,
           "prediction_horizon": 12, "temporal_seq_len": a.L_in, "num_years": 13}
    x, tf, y = synthetic_batch(a.batch, a.L_in, 2911, 6, 12)
    tf = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(a.batch, a.L_in, 2911, 4)   # stride 0 over the nodes
    x, y = x.to(dev), y.to(dev)
    ei = grid_graph()[0].to(dev)
    model = TEC_MoLLM(dict(cfg, gat_graphs="per_timestep", precision="fp32", include_wte=False,
                           load_pretrained_gpt2=False)).to(dev).train()

    def run(need_dx, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            model.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(need_dx)
            F_.HuberFn.apply(model(xi, tf, ei), y, 1.0).backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    run(True, 1)
    run(False, 1)
    with_dx = run(True, a.steps)
    without = run(False, a.steps)
    print(f"ms per forward + backward: {with_dx:.2f} with x.requires_grad, {without:.2f} without ({a.steps} steps each)")


if __name__ == "__main__":
    main()
