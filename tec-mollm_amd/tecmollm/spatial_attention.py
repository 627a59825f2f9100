"""What the GATv2 stage attends to: the attention coefficients of the spatial encoder, exported and scored on the device.

With PyG the reference's users get the coefficients from one keyword, `gat_conv(x, edge_index,
return_attention_weights=True)` (modules.py:329-336,:356).  Here the fused spatial kernels recompute them in every forward and
backward and keep none, so a kernel of its own forms them for the caller (`csrc/spatial_attn.hip`): alpha_ij says how much grid
cell i listens to neighbour j (within the graph's distance threshold) and to itself, per head, per (sample, timestep) graph --
before the attention dropout, i.e. what `eval()` uses and what training draws its masks over.

  * `spatial_attention(model, x, time_features, edge_index)` -> (edge_index_sl, alpha): the raw coefficients in PyG's edge
    order (the non-self edges as given, then one self loop per node);
  * `AttentionStats` / `evaluate_attention`: per group of graphs (storm level of the window, time of day of the timestep,
    lag inside the window) and per edge the mean, spread and message size of alpha, per node its self weight, the entropy of its
    attention row, how much the others listen to it and how far it is from plain neighbour averaging -- accumulated on the
    device in float64 with one owning thread per cell (the same calls give the same bits), one pass, no host synchronisation;
  * `attention_maps`, `write_attention`: the direction a cell listens in, and the files.

Edge orders: the kernel works in KERNEL ORDER (the by-target CSR entries, then the self loops); `GraphMeta.edge_pos` maps a CSR
entry to its position in the given edge list, which is how everything returned here is in PyG's order.
"""
from __future__ import annotations

import csv
import os
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, devcheck, ops
from . import functions as F_
from . import graph as graph_
from ._lib import TecmError
from .evaluate import check_grid
from .loop import _batches

HEADS = 2
EDGE_KEYS = ("mean", "std", "message", "uniform_gap")
NODE_KEYS = ("self_weight", "entropy", "effective_neighbours", "influence")


def _eval_plan() -> F_.DropPlan:
    return F_.DropPlan(training=False, p=0.0, base_seed=0)


def _gpu(t: torch.Tensor, name: str) -> None:
    _lib.require_gpu_tensor(t, name)


def _model_descriptor(model, x: torch.Tensor, tf: torch.Tensor, edge_index: torch.Tensor):
    """(descriptor, graph meta, tensors to keep alive) of the fused spatial stage as `TEC_MoLLM.forward` runs it."""
    _gpu(x, "x")
    _gpu(tf, "time_features")
    if x.dim() != 4 or tf.shape != (*x.shape[:3], 4):
        raise ValueError("x must be (B, L, N, C_in) and time_features (B, L, N, 4)")
    B, L, N, Cin = x.shape
    emb, enc = model.spatio_temporal_embedding, model.spatial_encoder
    if N != model.num_nodes or Cin != model.c_in:
        raise ValueError(f"x has (N, C_in) = ({N}, {Cin}), model was built for ({model.num_nodes}, {model.c_in})")
    x = x.detach().contiguous()
    meta = graph_.get(edge_index, N, x.device, emb.d_emb)
    R = 1 if model.gat_graphs == "reference" else B * L
    tensors = [t.detach() for t in (*emb.tables(), *enc.params())]
    d = F_.SpatialFn._desc(x, tf.detach(), *tensors, meta, model.heads, R, _eval_plan(), B, L, N, Cin, emb.d_emb)
    return d, meta, (x, tf, tensors)


def edge_index_with_self_loops(meta: "graph_.GraphMeta") -> torch.Tensor:
    """(2, E'') int64 on the device, PyG's order after `remove_self_loops` + `add_self_loops`: the non-self edges in their given
    order, then the self loops 0..N-1.  Built from the CSR without a host synchronisation."""
    N, E1 = meta.num_nodes, meta.num_edges
    dev = meta.rowptr.device
    loops = torch.arange(N, device=dev, dtype=torch.int64)
    if E1 == 0:
        return torch.stack([loops, loops])
    deg = (meta.rowptr[1:] - meta.rowptr[:-1]).to(torch.int64)
    tgt_csr = torch.repeat_interleave(loops, deg, output_size=E1)
    pos = meta.edge_pos[:E1].to(torch.int64)
    src = torch.empty(E1, device=dev, dtype=torch.int64)
    tgt = torch.empty(E1, device=dev, dtype=torch.int64)
    src[pos] = meta.colidx[:E1].to(torch.int64)
    tgt[pos] = tgt_csr
    return torch.stack([torch.cat([src, loops]), torch.cat([tgt, loops])])


def _perm(meta: "graph_.GraphMeta") -> Optional[torch.Tensor]:
    return meta.edge_pos if meta.num_edges > 0 else None


def _export(d, meta, max_ws_bytes: Optional[int] = None) -> torch.Tensor:
    """(B*L, E'', H) coefficients of descriptor `d` in PyG's order."""
    alpha = torch.empty(d.B * d.L, meta.num_edges + d.N, HEADS, device=meta.rowptr.device, dtype=torch.float32)
    errs = devcheck.error_word(alpha.device)
    ops.spatial_attention(d, meta.num_edges, alpha=alpha, perm=_perm(meta), max_ws_bytes=max_ws_bytes)
    errs.post()
    return alpha


@torch.no_grad()
def spatial_attention(model, x: torch.Tensor, time_features: torch.Tensor, edge_index: torch.Tensor, *,
                      max_ws_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The GATv2 attention coefficients of `model`'s spatial stage for one batch: (edge_index_sl, alpha) with edge_index_sl
    (2, E'') int64 in PyG's order (the non-self edges of `edge_index` as given, then the self loops 0..N-1; [0] = source j,
    [1] = target i) and alpha (B, L, E'', H) float32 on the device, alpha[b, t, e, h] = how much target i listens to source j
    in graph (b, t), head h.  Over the entries of one target the coefficients sum to 1.

    Two kernel launches per chunk of graphs, no GPT-2, no autograd; the coefficients are those before the attention dropout,
    whatever `model.training` says.  With `gat_graphs = "reference"` only graph (t = 0, b = 0) aggregates neighbours; every
    other graph has alpha = 1 on its self loops and 0 elsewhere.  A time index outside its table gives NaN coefficients and
    raises at the next `check_device_errors()`, as in the forward."""
    d, meta, keep = _model_descriptor(model, x, time_features, edge_index)
    alpha = _export(d, meta, max_ws_bytes)
    del keep
    return edge_index_with_self_loops(meta), alpha.view(d.B, d.L, meta.num_edges + d.N, HEADS)


@torch.no_grad()
def encoder_attention(encoder, x: torch.Tensor, edge_index: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The same for the stand-alone `SpatialEncoder` (x (num_graphs, N, 22), no embedding, no residual): (edge_index_sl,
    alpha (num_graphs, E'', H)) -- what `SpatialEncoder.forward(..., return_attention_weights=True)` returns next to `out`."""
    _gpu(x, "x")
    G, N, _ = x.shape
    meta = graph_.get(edge_index, N, x.device, 0)
    R = 1 if encoder.gat_graphs == "reference" else G
    xc = x.detach().contiguous()
    d = F_.GatFn._desc(xc, *[t.detach() for t in encoder.params()], meta, encoder.heads, R, _eval_plan())
    return edge_index_with_self_loops(meta), _export(d, meta)


# ------------------------------------------------------------------------------------ groups of graphs
def graph_groups_by_sample(sample_ids: torch.Tensor, L: int) -> torch.Tensor:
    """(B,) int32 ids of the batch's windows (e.g. `window_groups_by_index`: quiet / active / storm by Kp) -> (B, L) int32: every
    timestep's graph gets its window's id."""
    _lib.require_gpu_tensor(sample_ids, "sample_ids", torch.int32)
    return sample_ids.view(-1, 1).expand(-1, int(L)).contiguous()


def graph_groups_by_slot(time_features: torch.Tensor) -> torch.Tensor:
    """(B, L, N, 4) time features -> (B, L) int32: the time-of-day slot 0..11 (column 0, read at node 0) of each graph's own
    timestep."""
    return time_features[:, :, 0, 0].to(torch.int32).contiguous()


def graph_groups_by_lag(B: int, L: int, device: Union[str, torch.device] = "cuda") -> torch.Tensor:
    """(B, L) int32: the position t = 0..L-1 of each graph inside its input window."""
    return torch.arange(int(L), device=device, dtype=torch.int32).view(1, -1).expand(int(B), -1).contiguous()


# ------------------------------------------------------------------------------------ statistics
def derive(edge_stats: np.ndarray, node_stats: np.ndarray, counts: np.ndarray, edge_index_sl: np.ndarray,
           num_nodes: int) -> Dict[str, np.ndarray]:
    """(G, 3, E'', H) float64 sums [alpha, alpha^2, m] in PyG's order, (G, N, H) entropy sums and (G,) graph counts -> the dict
    `AttentionStats.compute` documents (with `edge_index_sl` itself).  Plain numpy."""
    es, ns = np.asarray(edge_stats, np.float64), np.asarray(node_stats, np.float64)
    n = np.asarray(counts, np.float64)
    G, _, E2, H = es.shape
    N, E1 = int(num_nodes), E2 - int(num_nodes)
    src, tgt = np.asarray(edge_index_sl[0], np.int64), np.asarray(edge_index_sl[1], np.int64)
    in_degree = np.bincount(tgt[:E1], minlength=N).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        nn_ = n.reshape(G, 1, 1)
        mean = es[:, 0] / nn_
        std = np.sqrt(np.maximum(es[:, 1] / nn_ - mean * mean, 0.0))
        message = es[:, 2] / nn_
        entropy = ns / nn_
    influence = np.zeros((G, N, H))
    for g in range(G):
        for h in range(H):
            influence[g, :, h] = np.bincount(src[:E1], weights=mean[g, :E1, h], minlength=N)
    out = {"count": n.copy(), "mean": mean, "std": std, "message": message,
           "self_weight": mean[:, E1:, :].copy(), "entropy": entropy, "effective_neighbours": np.exp(entropy),
           "influence": influence, "in_degree": in_degree, "edge_index_sl": np.stack([src, tgt]),
           "uniform_gap": mean - (1.0 / (in_degree[tgt] + 1.0)).reshape(1, E2, 1)}
    empty = n == 0
    for k in EDGE_KEYS + NODE_KEYS:
        out[k] = np.where(empty.reshape(G, 1, 1), np.nan, out[k])
    return out


class AttentionStats:
    """Running statistics of the attention coefficients per group of graphs: update(...) per batch on the device (the three
    launches of `tecm_spatial_attention`; fp64 sums, one owning thread per cell, no atomics: the same calls give the same
    bits), compute() at the end.  `num_edges_sl` is E'' = non-self edges + nodes."""

    def __init__(self, num_nodes: int, num_edges_sl: int, num_groups: int = 1, device: Union[str, torch.device] = "cuda"):
        self.N, self.E2, self.G = int(num_nodes), int(num_edges_sl), int(num_groups)
        if self.N < 1 or self.E2 < self.N or self.G < 1:
            raise ValueError("AttentionStats needs at least one node, one entry per node and one group")
        ne, nn_ = self.G * 3 * self.E2 * HEADS, self.G * self.N * HEADS
        self.stats = torch.zeros(ne + nn_, device=device, dtype=torch.float64)       # one buffer: one all-reduce
        self.edge_stats = self.stats[:ne].view(self.G, 3, self.E2, HEADS)           # kernel order
        self.node_stats = self.stats[ne:].view(self.G, self.N, HEADS)
        self.counts = torch.zeros(self.G, device=device, dtype=torch.int64)
        self.meta: Optional[graph_.GraphMeta] = None

    def reset(self) -> None:
        self.stats.zero_()
        self.counts.zero_()

    @torch.no_grad()
    def update(self, model, x: torch.Tensor, time_features: torch.Tensor, edge_index: torch.Tensor,
               groups: Optional[torch.Tensor] = None, skip_unconnected: bool = True, *,
               max_ws_bytes: Optional[int] = None) -> None:
        """Adds the (B*L) graphs of one batch.  `groups` (B, L) int32 on the device names each graph's group (None: group 0);
        an id outside [0, num_groups) skips that graph and raises `TecmError` at the next `check_device_errors()`.
        `skip_unconnected` leaves graphs without edges out of every sum: with `gat_graphs = "reference"` only graph
        (t = 0, b = 0) of a call aggregates neighbours, and a mean over the others would only dilute it."""
        d, meta, keep = _model_descriptor(model, x, time_features, edge_index)
        if d.N != self.N or meta.num_edges + d.N != self.E2:
            raise ValueError(f"graph has {d.N} nodes and {meta.num_edges + d.N} entries, the statistics {self.N} and {self.E2}")
        if groups is not None:
            _lib.require_gpu_tensor(groups, "groups", torch.int32)
            if tuple(groups.shape) != (d.B, d.L):
                raise ValueError(f"groups must hold one id per graph: {tuple(groups.shape)} for (B, L) = {(d.B, d.L)}")
            groups = groups.contiguous().view(-1)
        if self.meta is None:
            self.meta = meta                         # every update must come with the same graph: the sums are per edge
        errs = devcheck.error_word(self.stats.device)
        ops.spatial_attention(d, meta.num_edges, edge_stats=self.edge_stats, node_stats=self.node_stats, counts=self.counts,
                              groups=groups, skip_unconnected=skip_unconnected, max_ws_bytes=max_ws_bytes)
        errs.post()
        del keep

    def merge_(self, group=None) -> "AttentionStats":
        """Sum the statistics over the ranks of `group`, in place: one all-reduce of the float64 sums (and one of the G graph
        counts), as `MapMetrics.merge_`."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.stats, op=dist.ReduceOp.SUM, group=group)
            dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=group)
        return self

    def edge_stats_pyg(self) -> torch.Tensor:
        """The (G, 3, E'', H) sums in PyG's edge order (a copy)."""
        if self.meta is None or self.meta.num_edges == 0:
            return self.edge_stats.clone()
        out = self.edge_stats.clone()
        E1 = self.meta.num_edges
        out[:, :, self.meta.edge_pos[:E1].to(torch.int64)] = self.edge_stats[:, :, :E1]
        return out

    def compute(self) -> Dict[str, np.ndarray]:
        """numpy arrays, edges in PyG's order (`edge_index_sl`, (2, E'')), NaN in every cell of a group that saw no graph:
          count (G)                          graphs added per group
          mean, std, message (G, E'', H)     of alpha over the group's graphs; message = mean of alpha_ij * |x_l[j, head]|_2
          self_weight (G, N, H)              mean alpha of the node's self loop
          entropy (G, N, H)                  mean of -sum_j alpha_ij ln alpha_ij over the node's attention row
          effective_neighbours (G, N, H)     exp(entropy): 1 = listens to one source, deg + 1 = plain averaging
          influence (G, N, H)                sum over the out-edges j -> i of mean alpha_ij, self excluded: how much the others
                                             listen to j
          in_degree (N)                      non-self in-edges of every node
          uniform_gap (G, E'', H)            mean alpha_ij - 1 / (deg_i + 1): the distance from plain neighbour averaging"""
        if self.meta is None:
            raise ValueError("AttentionStats.compute() before any update()")
        ei = edge_index_with_self_loops(self.meta).cpu().numpy()
        return derive(self.edge_stats_pyg().cpu().numpy(), self.node_stats.cpu().numpy(), self.counts.cpu().numpy(), ei, self.N)


@torch.no_grad()
def evaluate_attention(model, dataset, edge_index: torch.Tensor, batch_size: int, groups=None,
                       num_groups: Optional[int] = None, order: Optional[Sequence[int]] = None, group=None,
                       skip_unconnected: bool = True) -> Dict[str, np.ndarray]:
    """`AttentionStats.compute()` of one pass over `dataset` (batches as in `evaluate_split`; no host synchronisation inside
    the pass).  `groups`: None (one group), "slot" (time-of-day slot of each graph's own timestep, 12 groups), "lag" (position
    inside the input window, L_in groups) or an int32 device tensor with one id in [0, num_groups) per DATASET index
    (`window_groups_by_index`), broadcast over the window's timesteps.  An id outside its range is skipped by the kernel and
    raises `TecmError` here.  `order` and `group` (the process group the statistics are summed over) as in `evaluate_split`."""
    by_index = isinstance(groups, torch.Tensor)
    if by_index and (groups.dtype != torch.int32 or groups.shape != (len(dataset),)):
        raise ValueError(f"groups must be an int32 tensor with one id per dataset index ({len(dataset)})")
    if not by_index and groups not in (None, "slot", "lag"):
        raise ValueError(f"groups must be None, 'slot', 'lag' or a tensor of ids, got {groups!r}")
    st: Optional[AttentionStats] = None
    for chunk in _batches(len(dataset), batch_size, order):
        x, tf, _ = dataset.batch(chunk)
        B, L, N, _c = x.shape
        if st is None:
            meta = graph_.get(edge_index, N, x.device, model.spatio_temporal_embedding.d_emb)
            G = int(num_groups) if num_groups is not None else {None: 1, "slot": 12, "lag": L}.get(None if by_index else groups, 1)
            st = AttentionStats(N, meta.num_edges + N, G, device=x.device)
        if by_index:
            ids = graph_groups_by_sample(groups[torch.as_tensor(chunk, dtype=torch.int64).to(groups.device, non_blocking=True)], L)
        elif groups == "slot":
            ids = graph_groups_by_slot(tf)
        elif groups == "lag":
            ids = graph_groups_by_lag(B, L, x.device)
        else:
            ids = None
        st.update(model, x, tf, edge_index, ids, skip_unconnected)
    if st is None:
        raise ValueError("evaluate_attention() on an empty dataset")
    out = st.merge_(group).compute()
    devcheck.check_device_errors(st.stats.device)
    return out


# ------------------------------------------------------------------------------------ maps and files
def grid_coords(grid: Sequence[int]) -> np.ndarray:
    """(rows * columns, 2) float64 (row, column) of every node id, ids taken row-major on the grid as `write_maps` does."""
    rows, cols = int(grid[0]), int(grid[1])
    r, c = np.divmod(np.arange(rows * cols), cols)
    return np.stack([r, c], axis=1).astype(np.float64)


def attention_maps(att: Dict[str, np.ndarray], grid: Optional[Sequence[int]] = (41, 71),
                   coords: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """`att` (an `AttentionStats.compute()` dict) plus `inflow_vector` (G, N, H, 2) = sum over the in-edges j -> i, self
    excluded, of mean alpha_ij * unit(coords_j - coords_i): the direction cell i listens in and how one-sided that is (0 for
    a symmetric neighbourhood with even weights).  `coords` (N, 2) places the nodes; without it they sit on `grid` = (rows,
    columns), ids row-major, and the two components run along the grid's rows and columns axes."""
    mean, ei = np.asarray(att["mean"]), np.asarray(att["edge_index_sl"])
    G, E2, H = mean.shape
    N = np.asarray(att["self_weight"]).shape[1]
    if coords is None:
        check_grid(grid, N)
        coords = grid_coords(grid)
    coords = np.asarray(coords, np.float64)
    if coords.shape != (N, 2):
        raise ValueError(f"coords must be ({N}, 2), got {coords.shape}")
    E1 = E2 - N
    src, tgt = ei[0, :E1], ei[1, :E1]
    delta = coords[src] - coords[tgt]
    length = np.linalg.norm(delta, axis=1, keepdims=True)
    unit = np.divide(delta, length, out=np.zeros_like(delta), where=length > 0)
    inflow = np.zeros((G, N, H, 2))
    for g in range(G):
        for h in range(H):
            for k in range(2):
                inflow[g, :, h, k] = np.bincount(tgt, weights=mean[g, :E1, h] * unit[:, k], minlength=N)
    out = dict(att)
    out["inflow_vector"] = np.where((np.asarray(att["count"]) == 0).reshape(G, 1, 1, 1), np.nan, inflow)
    return out


def write_attention(att: Dict[str, np.ndarray], output_dir: str, grid: Sequence[int] = (41, 71)) -> Dict[str, str]:
    """The files of an `evaluate_attention` result: `attention_maps.npz` -- the per-node fields (self_weight, entropy,
    effective_neighbours, influence) as (G, H, *grid), inflow_vector as (G, H, *grid, 2), the per-edge fields (mean, std,
    message, uniform_gap) as (G, E'', H) next to edge_index_sl (2, E''), in_degree as grid and count (G) -- and
    `attention_by_group.csv`: per group and head the graphs counted, the mean self weight, the mean effective neighbours and
    the mean |uniform_gap|.  numpy and the standard library only.  Returns the two paths."""
    if "inflow_vector" not in att:
        att = attention_maps(att, grid=grid)
    N = np.asarray(att["self_weight"]).shape[1]
    check_grid(grid, N)
    shape = [int(v) for v in grid]
    os.makedirs(output_dir, exist_ok=True)
    arrays = {"count": np.asarray(att["count"]), "edge_index_sl": np.asarray(att["edge_index_sl"]),
              "in_degree": np.asarray(att["in_degree"]).reshape(shape)}
    for k in NODE_KEYS:
        a = np.asarray(att[k])                                              # (G, N, H)
        arrays[k] = a.transpose(0, 2, 1).reshape(a.shape[0], a.shape[2], *shape)
    v = np.asarray(att["inflow_vector"])                                    # (G, N, H, 2)
    arrays["inflow_vector"] = v.transpose(0, 2, 1, 3).reshape(v.shape[0], v.shape[2], *shape, 2)
    for k in EDGE_KEYS:
        arrays[k] = np.asarray(att[k])
    npz_path = os.path.join(output_dir, "attention_maps.npz")
    np.savez_compressed(npz_path, **arrays)
    csv_path = os.path.join(output_dir, "attention_by_group.csv")
    with open(csv_path, "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow(["group", "head", "count", "self_weight_mean", "effective_neighbours_mean", "abs_uniform_gap_mean"])
        count = np.asarray(att["count"])
        for g in range(count.shape[0]):
            for h in range(HEADS):
                wr.writerow([g, h, int(count[g]), repr(float(np.mean(att["self_weight"][g, :, h]))),
                             repr(float(np.mean(att["effective_neighbours"][g, :, h]))),
                             repr(float(np.mean(np.abs(att["uniform_gap"][g, :, h]))))])
    return {"npz": npz_path, "csv": csv_path}


__all__ = ["spatial_attention", "encoder_attention", "AttentionStats", "evaluate_attention", "attention_maps",
           "write_attention", "graph_groups_by_sample", "graph_groups_by_slot", "graph_groups_by_lag", "derive",
           "edge_index_with_self_loops", "TecmError"]
