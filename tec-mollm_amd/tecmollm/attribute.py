"""Attribution of a forecast to its input: the gradient of the prediction with respect to `x`, integrated gradients, and
the maps and files made of them.

The reference is plain torch, so `x.requires_grad_()` followed by `backward()` gives `x.grad` there.  Here the gradient
passes the prediction head, the GPT-2 blocks and the temporal encoder as in a training step and reaches the input through
the fused spatial stage's input gradient (`csrc/spatial_dx.hip`: GATv2, the residual and the embedding concat, fp32 in every
precision mode, bit-reproducible).  Everything here runs with the parameters frozen, so no parameter gradient is formed.

`x` is the FEATURE-scaled input the model is trained on (channel 0 the TEC history, then the space-weather indices), so an
all-zero baseline is the standardised mean of every channel.
"""
from __future__ import annotations

import csv
import os
from contextlib import contextmanager
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .evaluate import check_grid


@contextmanager
def _frozen(model: torch.nn.Module, eval_mode: bool = False):
    """Every parameter's requires_grad off (and eval mode, if asked) inside the block; both restored afterwards."""
    flags = [(p, p.requires_grad) for p in model.parameters()]
    training = model.training
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        if eval_mode:
            model.eval()
        yield
    finally:
        for p, f in flags:
            p.requires_grad_(f)
        model.train(training)


def _index(sel, device) -> torch.Tensor:
    return torch.as_tensor(sel, dtype=torch.int64, device=device).reshape(-1)


def _select(t: torch.Tensor, horizons, nodes) -> torch.Tensor:
    """(B, L_out, N, 1) -> (B, horizons, nodes)."""
    t = t[..., 0]
    if horizons is not None:
        t = t.index_select(1, _index(horizons, t.device))
    if nodes is not None:
        t = t.index_select(2, _index(nodes, t.device))
    return t


def _grad_of_sum(model, x, tf, edge_index, horizons, nodes) -> torch.Tensor:
    xg = x.detach().requires_grad_(True)
    with torch.enable_grad():
        obj = _select(model(xg, tf, edge_index), horizons, nodes).sum()
        return torch.autograd.grad(obj, xg)[0]


def input_gradient(model: torch.nn.Module, x: torch.Tensor, tf: torch.Tensor, edge_index: torch.Tensor, *,
                   horizons: Optional[Sequence[int]] = None, nodes: Optional[Sequence[int]] = None,
                   y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d objective / d x, shape (B, L_in, N, C_in).  The objective is the sum of the predictions over the selected forecast
    horizons and nodes (all of them by default); with `y` (B, L_out, N, 1) it is the Huber loss (delta 1, mean) of the same
    selection.  The model runs in the mode it is in: in training mode its dropout masks are drawn as in a training step."""
    with _frozen(model):
        if y is None:
            return _grad_of_sum(model, x, tf, edge_index, horizons, nodes)
        xg = x.detach().requires_grad_(True)
        with torch.enable_grad():
            pred = _select(model(xg, tf, edge_index), horizons, nodes)
            loss = torch.nn.functional.huber_loss(pred, _select(y, horizons, nodes), delta=1.0)
            return torch.autograd.grad(loss, xg)[0]


def integrated_gradients(model: torch.nn.Module, x: torch.Tensor, tf: torch.Tensor, edge_index: torch.Tensor,
                         baseline: Optional[torch.Tensor] = None, steps: int = 16,
                         horizons: Optional[Sequence[int]] = None,
                         nodes: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Integrated gradients of F = sum of the selected predictions along the straight path from `baseline` (zeros: the
    standardised mean) to `x`, midpoint rule: attr = (x - x0) * mean_k dF/dx(x0 + (k + 1/2)/steps * (x - x0)), in eval mode.
    Returns (attr (B, L_in, N, C_in), delta (B,)) with delta = sum(attr) - (F(x) - F(x0)) per sample, the completeness gap:
    it shrinks as `steps` grows, and a gap that does not is a gradient that is not the function's."""
    if steps < 1:
        raise ValueError("steps must be at least 1")
    x = x.detach()
    x0 = torch.zeros_like(x) if baseline is None else baseline.detach().expand_as(x)
    diff = x - x0
    acc = torch.zeros_like(x)
    with _frozen(model, eval_mode=True):
        for k in range(steps):
            acc += _grad_of_sum(model, x0 + ((k + 0.5) / steps) * diff, tf, edge_index, horizons, nodes)
        with torch.no_grad():
            f1 = _select(model(x, tf, edge_index), horizons, nodes).sum(dim=(1, 2))
            f0 = _select(model(x0.contiguous(), tf, edge_index), horizons, nodes).sum(dim=(1, 2))
    attr = diff * (acc / steps)
    return attr, attr.sum(dim=(1, 2, 3)) - (f1 - f0)


def attribution_maps(attr: torch.Tensor, channel_names: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """|attr| (B, L_in, N, C_in) summed over what a map leaves out, averaged over the batch: `lag_channel` (L_in, C_in),
    `node_channel` (N, C_in), `channel` (C_in,), and `channel_names` (given, or "channel0" ..)."""
    if attr.dim() != 4:
        raise ValueError(f"attr must be (B, L_in, N, C_in), got {tuple(attr.shape)}")
    names = [f"channel{c}" for c in range(attr.shape[3])] if channel_names is None else [str(n) for n in channel_names]
    if len(names) != attr.shape[3]:
        raise ValueError(f"{len(names)} channel names for {attr.shape[3]} channels")
    a = attr.detach().abs()
    return {"lag_channel": a.sum(dim=2).mean(dim=0), "node_channel": a.sum(dim=1).mean(dim=0),
            "channel": a.sum(dim=(1, 2)).mean(dim=0), "channel_names": names}


def _numpy(v) -> np.ndarray:
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def write_attributions(maps: Dict[str, object], out_dir: str, grid: Optional[Sequence[int]] = None) -> Dict[str, str]:
    """The files of `attribution_maps`' result: `attributions.npz` with `lag_channel`, `node_channel` -- (*grid, C_in) when
    `grid`, e.g. (41, 71), is given -- and `channel`; `attribution_by_channel.csv` with one row per channel: its name, its
    attribution and its share of the total.  numpy and the standard library only.  Returns the two paths."""
    os.makedirs(out_dir, exist_ok=True)
    lag, node, chan = (_numpy(maps[k]) for k in ("lag_channel", "node_channel", "channel"))
    if grid is not None:
        check_grid(grid, node.shape[0])
        node = node.reshape(*[int(d) for d in grid], node.shape[1])
    npz_path = os.path.join(out_dir, "attributions.npz")
    np.savez_compressed(npz_path, lag_channel=lag, node_channel=node, channel=chan)
    csv_path = os.path.join(out_dir, "attribution_by_channel.csv")
    total = float(chan.sum())
    with open(csv_path, "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow(["channel", "attribution", "share"])
        for name, v in zip(maps["channel_names"], chan):
            wr.writerow([name, repr(float(v)), repr(float(v) / total if total > 0 else 0.0)])
    return {"npz": npz_path, "csv": csv_path}
