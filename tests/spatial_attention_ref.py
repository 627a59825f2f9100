"""float64 statements of the GATv2 attention coefficients and of what `tecmollm.spatial_attention` makes of them, shared by
tests/test_host_spatial_attention.py and tests/test_gpu_spatial_attention.py.  A helper, not a test.

`gat_attention` restates `oracle.ref_cpu.gatv2_conv` (PyG's GATv2Conv at the reference's call site, modules.py:329-336,:356)
up to the coefficients it does not return; tests/test_host_spatial_attention.py ties it back to the frozen oracle through
sum_j alpha_ij x_l[j] + bias.  `derive_ref`, `inflow_ref` and `accumulate_ref` are loop-by-loop numpy statements of
`AttentionStats.compute`, `attention_maps` and of the ordered fp64 accumulation of csrc/spatial_attn.hip."""
from __future__ import annotations

import numpy as np
import torch

from oracle import ref_cpu as R

NEG_SLOPE = 0.2
HEADS = 2


def gat_params64(p):
    """The six GATv2 tensors of an oracle parameter dict as float64 numpy: (Wl, bl, Wr, br, att (H, Ch), bias)."""
    get = lambda n: p[R.P_GAT + n].detach().double().cpu().numpy()           # noqa: E731
    att = get("att")
    return get("lin_l.weight"), get("lin_l.bias"), get("lin_r.weight"), get("lin_r.bias"), att.reshape(att.shape[-2:]), get("bias")


def edge_index_sl(edge_index, num_nodes: int) -> np.ndarray:
    """(2, E'') PyG's order: the non-self edges as given, then the self loops 0..N-1."""
    ei = np.asarray(edge_index, np.int64)
    keep = ei[0] != ei[1]
    loops = np.arange(num_nodes, dtype=np.int64)
    return np.stack([np.concatenate([ei[0][keep], loops]), np.concatenate([ei[1][keep], loops])])


def gat_attention(h, edge_index, p, use_edges: bool = True):
    """h (N, C) rows of ONE graph (any float type; computed in float64) -> (alpha (E'', H) in PyG's order, x_l (N, H, Ch),
    entropy (N, H), message (E'', H)).  use_edges False: the graph holds its self loops only, every other entry is 0."""
    Wl, bl, Wr, br, att, _ = gat_params64(p)
    h = np.asarray(h, np.float64)
    N = h.shape[0]
    H, Ch = att.shape
    xl = (h @ Wl.T + bl).reshape(N, H, Ch)
    xr = (h @ Wr.T + br).reshape(N, H, Ch)
    src, dst = edge_index_sl(edge_index, N)
    E2 = src.size
    live = np.ones(E2, bool) if use_edges else np.arange(E2) >= E2 - N
    s = xl[src] + xr[dst]
    e = (np.where(s > 0, s, NEG_SLOPE * s) * att[None]).sum(-1)             # (E'', H)
    alpha = np.zeros((E2, H))
    for i in range(N):
        rows = np.nonzero((dst == i) & live)[0]
        pe = np.exp(e[rows] - e[rows].max(axis=0, keepdims=True))
        alpha[rows] = pe / (pe.sum(axis=0, keepdims=True) + 1e-16)
    return alpha, xl, entropy_of(alpha, dst, N), alpha * np.linalg.norm(xl, axis=-1)[src]


def entropy_of(alpha, dst, num_nodes: int) -> np.ndarray:
    """(N, H): -sum_j alpha ln alpha over the entries of each target, entries with alpha = 0 contributing 0."""
    a = np.asarray(alpha, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(a == 0, 0.0, -a * np.log(a))
    out = np.zeros((num_nodes, a.shape[1]))
    np.add.at(out, dst, term)
    return out


def embed64(x, tf, p) -> np.ndarray:
    """The rows h = [x | node_emb + temporal_emb] (B, L, N, 22) of the fused stage in float64 (oracle.ref_cpu.embed)."""
    p64 = {k: v.double() for k, v in p.items() if k.startswith(R.P_EMB)}
    return R.embed(x.detach().double().cpu(), tf.detach().cpu(), p64).numpy()


def model_attention(x, tf, edge_index, p, graphs_with_edges: int):
    """Per graph (b, t) of the fused stage: alpha (B, L, E'', H), x_l (B, L, N, H, Ch), entropy (B, L, N, H), message
    (B, L, E'', H), float64.  Graph (b, t) has edges iff t*B + b < graphs_with_edges (the reference's flattening)."""
    h = embed64(x, tf, p)
    B, L = h.shape[:2]
    outs = [[gat_attention(h[b, t], edge_index, p, t * B + b < graphs_with_edges) for t in range(L)] for b in range(B)]
    return tuple(np.stack([np.stack([outs[b][t][k] for t in range(L)]) for b in range(B)]) for k in range(4))


# ------------------------------------------------------------------------------------ accumulation and derived fields
def accumulate_ref(alpha32, message, entropy, groups, num_groups: int, stats=None):
    """The kernel's accumulation, in its order: graphs in ascending order, each added to the float64 sums of its group.
    alpha32 (Gr, E'', H) float32 as exported; message (Gr, E'', H), entropy (Gr, N, H) any float; groups (Gr,) ids (outside
    [0, num_groups): the graph is skipped) or None.  Returns (edge (G, 3, E'', H), node (G, N, H), counts (G))."""
    a = np.asarray(alpha32)
    Gr, E2, H = a.shape
    N = np.asarray(entropy).shape[1]
    edge, node, counts = stats if stats is not None else (np.zeros((num_groups, 3, E2, H)), np.zeros((num_groups, N, H)),
                                                           np.zeros(num_groups, np.int64))
    for gr in range(Gr):
        g = 0 if groups is None else int(groups[gr])
        if not 0 <= g < num_groups:
            continue
        a64 = a[gr].astype(np.float64)
        edge[g, 0] += a64
        edge[g, 1] += a64 * a64
        edge[g, 2] += np.asarray(message[gr], np.float64)
        node[g] += np.asarray(entropy[gr], np.float64)
        counts[g] += 1
    return edge, node, counts


def derive_ref(edge, node, counts, ei_sl, num_nodes: int):
    """`AttentionStats.compute()`'s fields from the sums (edges in PyG's order), entry by entry."""
    G, _, E2, H = edge.shape
    N, E1 = num_nodes, E2 - num_nodes
    src, dst = ei_sl
    deg = np.zeros(N, np.int64)
    for e in range(E1):
        deg[dst[e]] += 1
    out = {k: np.full((G, E2, H), np.nan) for k in ("mean", "std", "message", "uniform_gap")}
    out.update({k: np.full((G, N, H), np.nan) for k in ("self_weight", "entropy", "effective_neighbours", "influence")})
    out["count"], out["in_degree"] = np.asarray(counts, np.float64), deg
    for g in range(G):
        n = float(counts[g])
        if n == 0:
            continue
        out["influence"][g] = 0.0
        for e in range(E2):
            mean = edge[g, 0, e] / n
            out["mean"][g, e] = mean
            out["std"][g, e] = np.sqrt(np.maximum(edge[g, 1, e] / n - mean * mean, 0.0))
            out["message"][g, e] = edge[g, 2, e] / n
            out["uniform_gap"][g, e] = mean - 1.0 / (deg[dst[e]] + 1)
            if e < E1:
                out["influence"][g, src[e]] += mean
            else:
                out["self_weight"][g, e - E1] = mean
        out["entropy"][g] = node[g] / n
        out["effective_neighbours"][g] = np.exp(node[g] / n)
    return out


def inflow_ref(mean, ei_sl, coords):
    """(G, N, H, 2): sum over the non-self in-edges j -> i of mean alpha_ij * unit(coords_j - coords_i)."""
    G, E2, H = mean.shape
    N = coords.shape[0]
    out = np.zeros((G, N, H, 2))
    for e in range(E2 - N):
        j, i = ei_sl[0][e], ei_sl[1][e]
        d = np.asarray(coords[j], np.float64) - np.asarray(coords[i], np.float64)
        if np.linalg.norm(d) > 0:
            out[:, i] += mean[:, e, :, None] * (d / np.linalg.norm(d))
    return out


def irregular_graph(num_nodes: int = 20, seed: int = 5) -> torch.Tensor:
    """(2, E) int64 edge list on `num_nodes` >= 12 nodes, in no particular order, with: a given self loop (3 -> 3), a duplicated
    edge (1 -> 2 twice), an isolated target (node 7: no in-edge, but out-edges) and a target of in-degree 10 (node 5)."""
    rng = np.random.default_rng(seed)
    edges = [(3, 3), (1, 2), (1, 2), (7, 0), (7, 4)] + [(j, 5) for j in range(6, 16)]
    for _ in range(3 * num_nodes):
        j, i = (int(v) for v in rng.integers(0, num_nodes, 2))
        if i not in (7, 5) and j != i:
            edges.append((j, i))
    order = rng.permutation(len(edges))
    return torch.tensor([edges[k] for k in order], dtype=torch.int64).t().contiguous()
