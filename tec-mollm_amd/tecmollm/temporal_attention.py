"""What the GPT-2 trunk attends to: the causal attention probabilities of every block, exported and scored on the device.

With Hugging Face the reference's users get them from one keyword, `GPT2Model(..., output_attentions=True)`
(modeling_gpt2.py:144-226, behind `LLMBackbone.forward`, modules.py:205-209): a (S, 12, T, T) tensor per block.  Here the
attention kernels form the softmax of every (sequence, head) in registers and keep only the context, and the lean forward
frees qkv as soon as the attention launch is queued, so a kernel of its own forms the probabilities from a tap on qkv
(`csrc/attention_probs.hip`, `DropPlan.attn_tap`): p[i, j] says how much patch token i of grid cell n listens to patch token
j <= i, per head, per block -- before the attention dropout, i.e. what `eval()` uses and what training draws its masks over.

  * `temporal_attention(model, x, time_features, edge_index)` -> (Ly, B, Ns, 12, T, T): the raw probabilities;
  * `TemporalAttentionStats` / `evaluate_temporal_attention`: per group of windows (storm level, ...), block, grid cell and head
    the mean row entropy, look-back distance, weight on token 0 (the attention sink) and weight on the token itself, per head
    the lag profile and (T <= 32) the mean matrix -- accumulated on the device in float64, no float atomics (the same calls
    give the same bits), one pass, no host synchronisation;
  * `write_temporal_attention`: the maps on the grid and the per-layer table.

This is the temporal twin of `tecmollm/spatial_attention.py`.
"""
from __future__ import annotations

import csv
import os
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib, devcheck, ops
from . import functions as F_
from ._lib import TecmError
from .evaluate import check_grid
from .loop import _batches

HEADS = F_.GPT_HEADS
NODE_KEYS = ("entropy", "lookback", "sink_weight", "self_weight")       # the order of node_stats' axis of 4
MAP_KEYS = NODE_KEYS + ("effective_tokens", "lookback_gap")


def _shape(model, x: torch.Tensor, time_features: torch.Tensor):
    if x.dim() != 4 or tuple(time_features.shape) != (*x.shape[:3], 4):
        raise ValueError("x must be (B, L, N, C_in) and time_features (B, L, N, 4)")
    return int(x.shape[0]), int(model.num_patches), int(model.num_nodes), int(model.llm_backbone.num_layers)


def _select_layers(layers: Optional[Sequence[int]], num_layers: int):
    sel = list(range(num_layers)) if layers is None else [int(v) for v in layers]
    if not sel or len(set(sel)) != len(sel) or any(v < 0 or v >= num_layers for v in sel):
        raise ValueError(f"layers must be distinct block indices in [0, {num_layers}), got {layers!r}")
    return sel


def _tapped_forward(model, x, time_features, edge_index, tap) -> torch.Tensor:
    """The eval-mode lean forward of `model` (no dropout at any site, `model.training` left as found) with `tap` on every
    GPT-2 block."""
    with F_.attention_tap(tap):
        return model(x, time_features, edge_index)


@torch.no_grad()
def temporal_attention(model, x: torch.Tensor, time_features: torch.Tensor, edge_index: torch.Tensor, *,
                       layers: Optional[Sequence[int]] = None, nodes: Union[None, Sequence[int], torch.Tensor] = None,
                       max_bytes: int = 1 << 30) -> torch.Tensor:
    """The causal attention probabilities of `model`'s GPT-2 blocks for one batch: attn (Ly_sel, B, Ns, 12, T, T) float32 on
    the device, attn[l, b, s, h, i, j] = how much patch token i listens to patch token j in block layers[l], window b, grid
    cell nodes[s], head h.  Rows sum to 1, entries j > i are exact zeros, row 0 is exactly [1, 0, ...].  `layers`: block
    indices (None: all); `nodes`: node ids (None: all N; an id outside [0, N) leaves its slot zero).

    Runs under no-grad as the eval-mode lean forward in the model's precision, whatever `model.training` says (the flag is
    left as found, no dropout is applied at any site); one extra launch per selected block.  An export larger than
    `max_bytes` raises ValueError: narrow it with `nodes=` or `layers=`."""
    B, T, N, Ly = _shape(model, x, time_features)
    sel = _select_layers(layers, Ly)
    Ns = N if nodes is None else int(len(nodes))
    nbytes = len(sel) * B * Ns * HEADS * T * T * 4
    if nbytes > int(max_bytes):
        raise ValueError(f"the export of {len(sel)} layers x {B} windows x {Ns} nodes x {HEADS} heads x {T} x {T} tokens takes "
                         f"{nbytes} bytes > max_bytes = {int(max_bytes)}: select fewer with nodes= or layers=, or raise max_bytes")
    _lib.require_gpu_tensor(x, "x")
    nodes_t = None
    if nodes is not None:
        if Ns < 1:
            raise ValueError("nodes= must name at least one node")
        nodes_t = torch.as_tensor(nodes).to(device=x.device, dtype=torch.int32).contiguous().view(-1)
    attn = torch.empty(len(sel), B, Ns, HEADS, T, T, device=x.device, dtype=torch.float32)
    slot = {layer: k for k, layer in enumerate(sel)}

    def tap(layer, qkv, B_, T_, N_):
        if layer in slot:
            ops.temporal_attention(qkv, B_, T_, N_, HEADS, qkv.shape[-1] // 3, probs=attn[slot[layer]], nodes=nodes_t)

    _tapped_forward(model, x, time_features, edge_index, tap)
    return attn


# ------------------------------------------------------------------------------------ statistics
def uniform_constants(T: int) -> Dict[str, float]:
    """Row-mean entropy and look-back of uniform causal attention p_ij = 1 / (i + 1): (1/T) sum_i ln(i + 1) and
    (1/T) sum_i i / 2."""
    i = np.arange(int(T), dtype=np.float64)
    return {"entropy_uniform": float(np.log(i + 1.0).sum() / T), "lookback_uniform": float((i / 2.0).sum() / T)}


def derive(node_stats: np.ndarray, lag_stats: np.ndarray, counts: np.ndarray,
           matrix_stats: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """(G, Ly, 4, N, H) float64 sums [entropy, look-back, sink, self], (G, Ly, H, T) lag sums, (G,) window counts and
    optionally (G, Ly, H, T, T) matrix sums -> the dict `TemporalAttentionStats.compute` documents.  Plain numpy."""
    ns, ls = np.asarray(node_stats, np.float64), np.asarray(lag_stats, np.float64)
    n = np.asarray(counts, np.float64)
    G, Ly, _, N, H = ns.shape
    T = ls.shape[-1]
    empty = n == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        per = ns / n.reshape(G, 1, 1, 1, 1)
        lag_profile = ls / (n.reshape(G, 1, 1, 1) * N * (T - np.arange(T, dtype=np.float64)).reshape(1, 1, 1, T))
    out: Dict[str, np.ndarray] = {"count": n.copy()}
    for k, name in enumerate(NODE_KEYS):
        out[name] = np.where(empty.reshape(G, 1, 1, 1), np.nan, per[:, :, k])
    out["effective_tokens"] = np.exp(out["entropy"])
    out["lag_profile"] = np.where(empty.reshape(G, 1, 1, 1), np.nan, lag_profile)
    if matrix_stats is not None:
        ms = np.asarray(matrix_stats, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["mean"] = np.where(empty.reshape(G, 1, 1, 1, 1), np.nan, ms / (n.reshape(G, 1, 1, 1, 1) * N))
    u = uniform_constants(T)
    out["entropy_uniform"] = np.float64(u["entropy_uniform"])
    out["lookback_uniform"] = np.float64(u["lookback_uniform"])
    out["lookback_gap"] = out["lookback"] - u["lookback_uniform"]
    return out


class TemporalAttentionStats:
    """Running statistics of the GPT-2 attention probabilities per group of windows: update(...) per batch on the device (one
    forward plus two launches of `tecm_temporal_attention` per block and chunk; fp64 sums, one owning thread per cell, no
    atomics: the same calls give the same bits), compute() at the end.  `matrix` (default: T <= 32) also keeps the mean
    (T, T) matrix per head."""

    def __init__(self, num_nodes: int, num_layers: int, T: int, num_groups: int = 1, matrix: Optional[bool] = None,
                 device: Union[str, torch.device] = "cuda"):
        self.N, self.Ly, self.T, self.G = int(num_nodes), int(num_layers), int(T), int(num_groups)
        if self.N < 1 or self.Ly < 1 or self.G < 1 or not 1 <= self.T <= 1024:
            raise ValueError("TemporalAttentionStats needs at least one node, layer and group and 1 <= T <= 1024")
        self.matrix = self.T <= 32 if matrix is None else bool(matrix)
        if self.matrix and self.T > 32:
            raise ValueError("the mean attention matrix is kept for T <= 32 only")
        nn_, nl = self.G * self.Ly * 4 * self.N * HEADS, self.G * self.Ly * HEADS * self.T
        nm = nl * self.T if self.matrix else 0
        self.stats = torch.zeros(nn_ + nl + nm, device=device, dtype=torch.float64)          # one buffer: one all-reduce
        self.node_stats = self.stats[:nn_].view(self.G, self.Ly, 4, self.N, HEADS)
        self.lag_stats = self.stats[nn_:nn_ + nl].view(self.G, self.Ly, HEADS, self.T)
        self.matrix_stats = self.stats[nn_ + nl:].view(self.G, self.Ly, HEADS, self.T, self.T) if self.matrix else None
        self.counts = torch.zeros(self.G, device=device, dtype=torch.int64)

    def reset(self) -> None:
        self.stats.zero_()
        self.counts.zero_()

    @torch.no_grad()
    def update(self, model, x: torch.Tensor, time_features: torch.Tensor, edge_index: torch.Tensor,
               groups: Optional[torch.Tensor] = None, *, max_ws_bytes: Optional[int] = None) -> torch.Tensor:
        """Adds the B windows of one batch and returns the model's predictions of that (eval-mode, no-grad) forward.
        `groups` (B,) int32 on the device names each window's group (None: group 0); an id outside [0, num_groups) skips
        that window in every sum and raises `TecmError` at the next `check_device_errors()`.  The window counts advance
        once per update (block 0's call counts)."""
        B, T, N, Ly = _shape(model, x, time_features)
        if (N, Ly, T) != (self.N, self.Ly, self.T):
            raise ValueError(f"the model has (N, layers, T) = {(N, Ly, T)}, the statistics {(self.N, self.Ly, self.T)}")
        _lib.require_gpu_tensor(x, "x")
        if groups is not None:
            _lib.require_gpu_tensor(groups, "groups", torch.int32)
            if tuple(groups.shape) != (B,):
                raise ValueError(f"groups must hold one id per window: {tuple(groups.shape)} for B = {B}")
            groups = groups.contiguous()
        errs = devcheck.error_word(self.stats.device)

        def tap(layer, qkv, B_, T_, N_):
            ops.temporal_attention(qkv, B_, T_, N_, HEADS, qkv.shape[-1] // 3, node_stats=self.node_stats,
                                   lag_stats=self.lag_stats, matrix_stats=self.matrix_stats, counts=self.counts, groups=groups,
                                   layer=layer, count=layer == 0, err_flag=errs.ptr(), max_ws_bytes=max_ws_bytes)

        pred = _tapped_forward(model, x, time_features, edge_index, tap)
        errs.post()
        return pred

    def merge_(self, group=None) -> "TemporalAttentionStats":
        """Sum the statistics over the ranks of `group`, in place: one all-reduce of the float64 sums (and one of the G window
        counts), as `AttentionStats.merge_`."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.stats, op=dist.ReduceOp.SUM, group=group)
            dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=group)
        return self

    def compute(self) -> Dict[str, np.ndarray]:
        """numpy arrays, NaN in every cell of a group that saw no window:
          count (G)                                     windows added per group
          entropy, lookback, sink_weight, self_weight   (G, Ly, N, H): means over the group's windows of the sequence's row means
                                                        of -sum_j p ln p, sum_j p (i - j) [tokens], p_i0 and p_ii
          effective_tokens (G, Ly, N, H)                exp(entropy): 1 = listens to one token
          lag_profile (G, Ly, H, T)                     mean p_{i,i-d} over windows, nodes and the T - d rows that have lag d
          mean (G, Ly, H, T, T)                         mean p_ij over windows and nodes (when the matrix is kept)
          entropy_uniform, lookback_uniform             the same row means for uniform causal attention p_ij = 1 / (i + 1)
          lookback_gap (G, Ly, N, H)                    lookback - lookback_uniform: < 0 = looks back less far than averaging"""
        return derive(self.node_stats.cpu().numpy(), self.lag_stats.cpu().numpy(), self.counts.cpu().numpy(),
                      self.matrix_stats.cpu().numpy() if self.matrix else None)


@torch.no_grad()
def evaluate_temporal_attention(model, dataset, edge_index: torch.Tensor, batch_size: int,
                                groups: Optional[torch.Tensor] = None, num_groups: Optional[int] = None,
                                order: Optional[Sequence[int]] = None, group=None) -> Dict[str, np.ndarray]:
    """`TemporalAttentionStats.compute()` of one pass over `dataset` (batches as in `evaluate_split`; no host synchronisation
    inside the pass).  `groups`: None (one group) or an int32 device tensor with one id in [0, num_groups) per DATASET index
    (`window_groups_by_index`).  An id outside its range is skipped by the kernel and raises `TecmError` here.  `order` and
    `group` (the process group the statistics are summed over) as in `evaluate_split`."""
    if groups is not None:
        if not isinstance(groups, torch.Tensor) or groups.dtype != torch.int32 or tuple(groups.shape) != (len(dataset),):
            raise ValueError(f"groups must be an int32 tensor with one id per dataset index ({len(dataset)})")
        if num_groups is None:
            raise ValueError("groups= needs num_groups=")
    st: Optional[TemporalAttentionStats] = None
    for chunk in _batches(len(dataset), batch_size, order):
        x, tf, _ = dataset.batch(chunk)
        if st is None:
            st = TemporalAttentionStats(model.num_nodes, model.llm_backbone.num_layers, model.num_patches,
                                        int(num_groups) if groups is not None else 1, device=x.device)
        ids = None
        if groups is not None:
            ids = groups[torch.as_tensor(chunk, dtype=torch.int64).to(groups.device, non_blocking=True)].contiguous()
        st.update(model, x, tf, edge_index, ids)
    if st is None:
        raise ValueError("evaluate_temporal_attention() on an empty dataset")
    out = st.merge_(group).compute()
    devcheck.check_device_errors(st.stats.device)
    return out


# ------------------------------------------------------------------------------------ files
def write_temporal_attention(att: Dict[str, np.ndarray], output_dir: str, grid: Sequence[int] = (41, 71)) -> Dict[str, str]:
    """The files of an `evaluate_temporal_attention` result: `temporal_attention_maps.npz` -- the per-node fields (entropy,
    lookback, sink_weight, self_weight, effective_tokens, lookback_gap) as (G, Ly, H, *grid), lag_profile (G, Ly, H, T), mean
    (G, Ly, H, T, T) when present, count (G) and the two uniform constants -- and `temporal_attention_by_layer.csv`: per group,
    layer and head the windows counted, the mean entropy, the mean look-back and its gap, the mean sink and self weight.
    numpy and the standard library only.  Returns the two paths."""
    ent = np.asarray(att["entropy"])
    G, Ly, N, H = ent.shape
    check_grid(grid, N)
    shape = [int(v) for v in grid]
    os.makedirs(output_dir, exist_ok=True)
    arrays = {"count": np.asarray(att["count"]), "lag_profile": np.asarray(att["lag_profile"]),
              "entropy_uniform": np.asarray(att["entropy_uniform"]), "lookback_uniform": np.asarray(att["lookback_uniform"])}
    if "mean" in att:
        arrays["mean"] = np.asarray(att["mean"])
    for k in MAP_KEYS:
        a = np.asarray(att[k])                                              # (G, Ly, N, H)
        arrays[k] = a.transpose(0, 1, 3, 2).reshape(G, Ly, H, *shape)
    npz_path = os.path.join(output_dir, "temporal_attention_maps.npz")
    np.savez_compressed(npz_path, **arrays)
    csv_path = os.path.join(output_dir, "temporal_attention_by_layer.csv")
    with open(csv_path, "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow(["group", "layer", "head", "count", "entropy_mean", "lookback_mean", "lookback_gap_mean", "sink_weight_mean",
                     "self_weight_mean"])
        count = np.asarray(att["count"])
        for g in range(G):
            for l in range(Ly):
                for h in range(H):
                    wr.writerow([g, l, h, int(count[g])] +
                                [repr(float(np.mean(np.asarray(att[k])[g, l, :, h])))
                                 for k in ("entropy", "lookback", "lookback_gap", "sink_weight", "self_weight")])
    return {"npz": npz_path, "csv": csv_path}


__all__ = ["temporal_attention", "TemporalAttentionStats", "evaluate_temporal_attention", "write_temporal_attention", "derive",
           "uniform_constants", "TecmError"]
