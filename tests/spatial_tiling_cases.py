"""Cases of the tiled spatial kernels (csrc/spatial_fwd.hip, spatial_fwd2.hip, spatial_bwd.hip <1> / <2>, spatial_bwd2.hip) over
every tiling tecmollm/graph.py:build can choose, CPU only: seeded graphs, the tiling and the entry points each one is expected
to get (tests/test_host_spatial_tiling.py pins both through the library), plain-Python restatements of the per-tile lists, and
the oracle runs shared by the host and the GPU tests (tests/test_gpu_spatial_tiling.py).

Graphs.  `banded(N, lo, hi)`: target i has the sources i - lo, i + hi and four seeded draws from [i - lo, i + hi]; ids outside
[0, N) and self loops are dropped, duplicates kept, edges listed target by target.  Every tile of tn nodes then has a window of
tn + lo + hi rows inside the graph, so (lo, hi) picks the rung of graph.TILE_SIZES: build takes the largest tile whose windows
fit the LDS and prefers windows of at most 256 rows.  `dense(N, b, deg)`: deg draws from [i - b, i + b] per target, the regime
where the edge arrays, not the window, fill the LDS.  `extra` appends single (source, target) edges to either.

A case names its tiling (tile_nodes, num_tiles, win_max, tile_edges_max) and its entry points as literals: what graph.build
and the library's predicates must return for it."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from oracle import ref_cpu as R

LDS_BUDGET = 160 * 1024
MAXI = 40                                                  # items a block of the first formulation may own
SPATIAL = [R.P_EMB + f"{n}_embedding.weight" for n in ("node", "tod", "doy", "year", "season")] + \
          [R.P_GAT + n for n in ("lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "att", "bias")]
MODES = ("reference", "per_timestep")
DROP_SEED = 24681357                                       # base seed of the alpha-dropout plan of the training-mode runs

FWD2, FWD1, BWD2, BWD1 = "tecm_spatial_fwd2", "tecm_spatial_fwd", "tecm_spatial_bwd2", "tecm_spatial_bwd"
ENTRY_POINTS = (FWD2, FWD1, BWD2, BWD1)

# gen: "band" (a, b) = (lo, hi) | "dense" (a, b) = (half width, draws per target);  tiling = (tile_nodes, num_tiles, win_max,
# tile_edges_max);  fwd / bwd: the entry points that serve the call by default;  cross: also run with the other Cin
Case = namedtuple("Case", "name gen a b extra N B L cin tiling fwd bwd seed cross", defaults=(0, False))


def banded(N: int, lo: int, hi: int, seed: int = 0, extra=()) -> torch.Tensor:
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for i in range(N):
        for j in [i - lo, i + hi] + rng.integers(i - lo, i + hi + 1, size=4).tolist():
            if 0 <= j < N and j != i:
                src.append(j)
                dst.append(i)
    for j, i in extra:
        src.append(j)
        dst.append(i)
    return torch.tensor([src, dst], dtype=torch.int64)


def dense(N: int, b: int, deg: int, seed: int = 0, extra=()) -> torch.Tensor:
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for i in range(N):
        for j in rng.integers(i - b, i + b + 1, size=deg).tolist():
            if 0 <= j < N and j != i:
                src.append(j)
                dst.append(i)
    for j, i in extra:
        src.append(j)
        dst.append(i)
    return torch.tensor([src, dst], dtype=torch.int64)


_W = (FWD1, BWD1)           # a window above 256 rows: the first formulation, its backward in two by-source rounds (<2>)
_V2 = (FWD2, BWD2)          # at most 256 rows and a second-formulation backward map within 80 KiB
CASES = (
    # ---- windows of exactly 256 rows: the five tile sizes both formulations serve
    Case("t128_w256", "band", 64, 64, (), 640, 2, 2, 6, (128, 5, 256, 765), *_V2),
    Case("t120_w256_odd", "band", 68, 68, (), 640, 1, 3, 10, (120, 6, 256, 719), *_V2, cross=True),
    Case("t112_w256", "band", 72, 72, (), 640, 2, 2, 6, (112, 6, 256, 670), *_V2),
    Case("t104_w256", "band", 76, 76, (), 640, 2, 2, 10, (104, 7, 256, 621), *_V2),
    Case("t96_w256", "band", 80, 80, (), 640, 2, 2, 6, (96, 7, 256, 574), *_V2),
    # a last tile of one node (N = 4 * 128 + 1)
    Case("t128_w256_last1", "band", 64, 64, (), 513, 2, 2, 10, (128, 5, 256, 765), *_V2),
    # ---- 257 rows: one edge 383 -> 639 widens the last tile's window by one row at every tile size, so build keeps 128; the
    #      second by-source round owns exactly one row, the target 639 itself
    Case("t128_w257", "band", 64, 64, ((383, 639),), 640, 2, 2, 6, (128, 5, 257, 765), *_W),
    # ---- wide windows: every rung of the ladder
    Case("t128_w292", "band", 82, 82, (), 640, 2, 2, 10, (128, 5, 292, 765), *_W),
    Case("t120_w312_odd", "band", 96, 96, (), 640, 1, 3, 6, (120, 6, 312, 719), *_W, cross=True),
    Case("t112_w323_budget", "band", 105, 106, (), 640, 2, 2, 10, (112, 6, 323, 671), *_W),   # forward LDS = the budget
    Case("t110_w322", "band", 106, 106, (), 640, 2, 2, 6, (110, 6, 322, 659), *_W),
    Case("t104_w324", "band", 110, 110, (), 640, 2, 2, 10, (104, 7, 324, 622), *_W),
    Case("t96_w332", "band", 118, 118, (), 640, 2, 2, 6, (96, 7, 332, 574), *_W),
    Case("t80_w340", "band", 130, 130, (), 640, 2, 2, 10, (80, 8, 340, 480), *_W),
    Case("t64_w348", "band", 142, 142, (), 640, 2, 2, 6, (64, 10, 348, 384), *_W),
    Case("t48_w360", "band", 156, 156, (), 640, 2, 2, 10, (48, 14, 360, 288), *_W),
    Case("t32_w368", "band", 168, 168, (), 640, 2, 2, 6, (32, 20, 368, 192), *_W),
    Case("t16_w380", "band", 182, 182, (), 640, 2, 2, 10, (16, 40, 380, 96), *_W),
    # tiles below one MFMA row block, B * L * num_tiles > 256: blocks own several items and switch tile inside
    Case("t8_w384", "band", 188, 188, (), 640, 2, 2, 6, (8, 80, 384, 48), *_W),
    Case("t4_w384", "band", 190, 190, (), 640, 1, 2, 10, (4, 160, 384, 24), *_W),
    Case("t2_w388", "band", 193, 193, (), 640, 1, 1, 10, (2, 320, 388, 12), *_W),          # the widest window, Cin = 10
    Case("t2_w388_odd", "band", 193, 193, (), 640, 1, 3, 6, (2, 320, 388, 12), *_W),
    # B * L * num_tiles = 10880 > 256 * MAXI: both launchers of the first formulation size their blocks at MAXI items
    Case("t1_w388_maxi", "band", 193, 194, (), 640, 1, 17, 10, (1, 640, 388, 6), *_W),
    # ---- many edges per tile (N = 200): the second backward's 80 KiB line, the first backward's 160 KiB
    Case("dense_under_bwd2", "dense", 20, 13, (), 200, 2, 2, 6, (128, 2, 146, 1555), *_V2),
    Case("dense_over_bwd2", "dense", 20, 14, (), 200, 2, 2, 10, (128, 2, 147, 1671), FWD2, BWD1),
    Case("dense_bwd_lds", "dense", 40, 20, (), 200, 1, 3, 6, (120, 2, 159, 2172), FWD2, BWD1),
)
BY_NAME = {c.name: c for c in CASES}
REFUSED = ("band", 194, 194, 640)                          # the first banded graph no one-node tile holds


def edges(c: Case) -> torch.Tensor:
    return (banded if c.gen == "band" else dense)(c.N, c.a, c.b, extra=c.extra)


def variants(c: Case):
    """The (case, Cin) pairs a test runs: the case's own Cin, and the other one where the case is marked `cross`."""
    return [(c, c.cin)] + ([(c, 16 - c.cin)] if c.cross else [])


def _h():
    import os
    from tecmollm import _lib
    if not os.path.exists(_lib.LIB_PATH):                  # as tests/test_host.py::built_lib
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


_meta_cache: Dict[Tuple[str, int], object] = {}


def meta_of(c: Case, cin: Optional[int] = None):
    """graph.build on the CPU for the case at d_emb = 22 - Cin."""
    from tecmollm import graph as G
    cin = c.cin if cin is None else cin
    if (c.name, cin) not in _meta_cache:
        _h()
        _meta_cache[(c.name, cin)] = G.build(edges(c), c.N, torch.device("cpu"), 22 - cin)
    return _meta_cache[(c.name, cin)]


_live = (C.c_float * 4)()


def descriptor(c: Case, meta, cin: Optional[int] = None):
    """The TecmSpatial of the case as SpatialFn fills it (block-uniform time features, 24-float output rows); pointers are live
    dummies: only the host predicates read it."""
    from tecmollm import _lib
    cin = c.cin if cin is None else cin
    d = _lib.TecmSpatial()
    d.B, d.L, d.N, d.Cin, d.Demb, d.H = c.B, c.L, c.N, cin, 22 - cin, 2
    d.graphs_with_edges, d.year_rows = c.B * c.L, 13
    d.num_tiles, d.tile_nodes, d.win_max, d.tile_edges_max = meta.num_tiles, meta.tile_nodes, meta.win_max, meta.tile_edges_max
    for name in ("x", "tf", "node_tab", "tod_tab", "doy_tab", "year_tab", "season_tab", "Wl", "bl", "Wr", "br", "att", "bias",
                 "rowptr", "colidx", "tile_lo", "tile_hi", "err_flag"):
        setattr(d, name, C.addressof(_live))
    d.tf_sb, d.tf_sl, d.tf_sn, d.tf_sf = c.L * 4, 4, 0, 1
    d.flags, d.out_ld = 0, 24
    return d


def routes(c: Case, meta, cin: Optional[int] = None) -> Tuple[str, str]:
    """The entry points SpatialFn takes by default, from the library's two predicates."""
    d = descriptor(c, meta, cin)
    h = _h()
    return (FWD2 if h.tecm_spatial_fwd2_ws_floats(C.byref(d)) > 0 else FWD1,
            BWD2 if h.tecm_spatial_bwd2_blocks(C.byref(d)) > 0 else BWD1)


def kernels(c: Case, v2: bool) -> Tuple[str, str]:
    """The kernels that serve the case, by name: default selection (v2) or the first formulation alone."""
    wide = c.tiling[2] > 256
    fwd = "spatial_fwd2" if v2 and c.fwd == FWD2 else "spatial_fwd"
    bwd = "spatial_bwd2" if v2 and c.bwd == BWD2 else ("spatial_bwd<2>" if wide else "spatial_bwd<1>")
    return fwd, bwd


# ------------------------------------------------------------------------------------ plain-Python restatements
def brute_tiles(edge_index: np.ndarray, num_nodes: int, tile_nodes: int):
    """Per tile, from the edge list alone: (lo, hi) of the window that holds the tile and every source of its targets, and the
    tile's edges in by-target order [(target, source), ...] (targets ascending, the given order inside a target)."""
    lists = [[] for _ in range(num_nodes)]
    for j, i in zip(edge_index[0].tolist(), edge_index[1].tolist()):
        if j != i:
            lists[i].append(j)
    out = []
    for n0 in range(0, num_nodes, tile_nodes):
        n1 = min(num_nodes, n0 + tile_nodes)
        seg = [(i, j) for i in range(n0, n1) for j in lists[i]]
        lo = min([n0] + [j for _, j in seg])
        hi = max([n1] + [j + 1 for _, j in seg])
        out.append((lo, hi, seg))
    return out


def brute_by_source_tile(lo: int, hi: int, n0: int, seg):
    """One tile's by-source list: for every window row w in [0, hi - lo) the edges that leave node lo + w, as codes
    ((target - n0) << 16) | position of the edge in `seg`, ordered by position.  Returns (ptr (W + 1), codes)."""
    rows = [[] for _ in range(hi - lo)]
    for pos, (i, j) in enumerate(seg):
        rows[j - lo].append(((i - n0) << 16) | pos)
    ptr = [0]
    for r in rows:
        ptr.append(ptr[-1] + len(r))
    return ptr, [code for r in rows for code in r]


# ------------------------------------------------------------------------------------ inputs and oracle runs
def stage_inputs(c: Case, cin: int):
    """(parameters of the stage, x (B, L, N, Cin), tf (B, L, N, 4) constant over the nodes, gout (B, L, N, 22)), seeded by the
    case."""
    seed = 1000 + 7 * CASES.index(c) + c.seed
    cfg = R.default_config(num_nodes=c.N, c_in=cin, d_emb=22 - cin)
    p = {k: v for k, v in R.init_params(cfg, seed=seed).items() if k.startswith((R.P_EMB, R.P_GAT))}
    x, tf, _ = R.synthetic_batch(c.B, c.L, c.N, cin, 12, seed=seed + 1)
    gout = torch.randn(c.B, c.L, c.N, 22, generator=torch.Generator().manual_seed(seed + 2))
    return p, x, tf, gout


_mask_cache: Dict[Tuple[str, str], torch.Tensor] = {}


def gat_masks(c: Case, mode: str) -> torch.Tensor:
    """The alpha-dropout multipliers of one training-mode forward with DropPlan(True, 0.1, DROP_SEED), in the oracle's edge
    order (tests/parity.py:device_masks; the other sites are shrunk to nothing)."""
    from tests.parity import device_masks
    if (c.name, mode) not in _mask_cache:
        mcfg = dict(R.default_config(num_nodes=c.N), temporal_seq_len=c.L, temporal_strides=[1, 1], patch_len=1, llm_layers=0,
                    d_llm=4)
        _mask_cache[(c.name, mode)] = device_masks(mcfg, c.B, edges(c), DROP_SEED, mode)["gat"]
    return _mask_cache[(c.name, mode)]


_oracle_cache: Dict[tuple, dict] = {}


def oracle(c: Case, cin: int, mode: str, train: bool, dtype=torch.float32) -> dict:
    """embed + GATv2 + residual of the case on the CPU oracle in `dtype`, and autograd through it for a seeded gout:
    {"out" (B, L, N, 22), "dx" (B, L, N, Cin), every name of SPATIAL: its gradient}.  One run per key, kept and not modified."""
    key = (c.name, cin, mode, train, dtype)
    if key not in _oracle_cache:
        p, x, tf, gout = stage_inputs(c, cin)
        mult = gat_masks(c, mode).to(dtype) if train else None
        pr = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
        xr = x.to(dtype).clone().requires_grad_(True)
        ref = R.spatial(R.embed(xr, tf, pr), edges(c), pr, 2, 1 if mode == "reference" else None, alpha_mult=mult)
        ref = ref.view(c.L, c.B, c.N, 22).permute(1, 0, 2, 3)
        grads = torch.autograd.grad(ref, [xr] + [pr[n] for n in SPATIAL], gout.to(dtype))
        res = {"out": ref.detach(), "dx": grads[0]}
        res.update(zip(SPATIAL, grads[1:]))
        _oracle_cache[key] = res
    return _oracle_cache[key]
