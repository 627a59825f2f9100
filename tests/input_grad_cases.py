"""Graphs and oracle runs shared by tests/test_host_input_grad.py and tests/test_gpu_input_grad.py."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from oracle import ref_cpu as R

# (rows, columns, threshold_km) -> what graph.build makes of it (tests/test_host_input_grad.py pins the windows):
GRID_ONE_TILE = (3, 4, 170.0)        # N = 12: one tile
GRID_TWO_TILES = (9, 15, 170.0)      # N = 135: two tiles of 128 / 7 targets, the smallest shape with cross-tile sources
GRID_WIDE = (3, 140, 170.0)          # N = 420: seven tiles, 256 < win_max = 346 <= 512 (the forward's first kernel)
NO_IN, NO_OUT = 40, 77               # nodes of the asymmetric graph without in-edges / without out-edges


def grid_edges(grid: Tuple[int, int, float]) -> torch.Tensor:
    return R.grid_graph(grid[0], grid[1], threshold_km=grid[2])[0]


def asymmetric_edges(seed: int = 5) -> torch.Tensor:
    """The 9 x 15 grid with a seeded half of its directed edges dropped, five explicit self loops added (the layer strips
    them and adds its own), node NO_IN left without in-edges and node NO_OUT without out-edges."""
    ei = grid_edges(GRID_TWO_TILES)
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(ei.shape[1], generator=g) < 0.5
    keep &= (ei[1] != NO_IN) & (ei[0] != NO_OUT)
    loops = torch.tensor([0, 7, NO_IN, NO_OUT, 134], dtype=torch.int64)
    return torch.cat([ei[:, keep], torch.stack([loops, loops])], 1)


def brute_by_source(edge_index: np.ndarray, num_nodes: int):
    """(out_ptr, out_target, out_slot) in plain Python: per target the given non-self edges in the given order (their
    position = the slot), then per source its entries ordered by target, ties by slot."""
    lists = [[] for _ in range(num_nodes)]                     # per target: sources in the given order
    for j, i in zip(edge_index[0].tolist(), edge_index[1].tolist()):
        if j != i:
            lists[i].append(j)
    out = [[] for _ in range(num_nodes)]
    for i, srcs in enumerate(lists):
        for slot, j in enumerate(srcs):
            out[j].append((i, slot))
    ptr = np.zeros(num_nodes + 1, dtype=np.int64)
    for j in range(num_nodes):
        ptr[j + 1] = ptr[j] + len(out[j])
    flat = [e for j in range(num_nodes) for e in sorted(out[j])]
    return ptr, np.asarray([e[0] for e in flat], dtype=np.int64), np.asarray([e[1] for e in flat], dtype=np.int64)


def oracle_stage_dx(p: Dict[str, torch.Tensor], x: torch.Tensor, tf: torch.Tensor, ei: torch.Tensor, gwe: Optional[int],
                    gout: torch.Tensor, alpha_mult: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d x of <gout, embed + GATv2 + residual> on the oracle: x, gout time-major (B, L, N, *)."""
    B, L, N, _ = x.shape
    xr = x.clone().requires_grad_(True)
    ref = R.spatial(R.embed(xr, tf, p), ei, p, 2, gwe, alpha_mult=alpha_mult).view(L, B, N, 22).permute(1, 0, 2, 3)
    return torch.autograd.grad(ref, xr, gout)[0]


def oracle_model_dx(cfg, params, x, tf, ei, y, gwe, masks=None, q: "R.Rounding" = R.FP32):
    """Huber-loss step of the oracle with x requiring grad: (dx, {trainable parameter: gradient})."""
    p = {k: v.clone().requires_grad_(R.is_trainable(k)) for k, v in params.items()}
    xr = x.clone().requires_grad_(True)
    loss = R.huber(R.forward(xr, tf, ei, p, cfg, gwe, q=q, masks=masks), y)
    names = [k for k, v in p.items() if v.requires_grad]
    grads = torch.autograd.grad(loss, [xr] + [p[k] for k in names], allow_unused=True)
    return grads[0], {k: (g if g is not None else torch.zeros_like(p[k])) for k, g in zip(names, grads[1:])}
