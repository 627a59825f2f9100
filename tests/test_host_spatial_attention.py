"""CPU tests of the host side of the spatial attention maps: the float64 reference (tests/spatial_attention_ref.py) against the
frozen oracle, `GraphMeta.edge_pos`, the derived fields of `AttentionStats.compute` / `attention_maps` on a 3-node case worked
out by hand, empty groups, the C ABI entries and the files `write_attention` writes.  No GPU."""
import ctypes
import os
import re

import numpy as np
import torch

from oracle import ref_cpu as R
from tests import parity
from tests import spatial_attention_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gat_params(seed=0):
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=20)
    return {k: v.double() for k, v in R.init_params(cfg, seed=seed).items() if k.startswith(R.P_GAT)}


def test_reference_reproduces_the_oracle_gatv2():
    """sum_j alpha_ij x_l[j] + bias from the helper equals oracle.ref_cpu.gatv2_conv (float64 on both sides) to rounding, on
    the irregular graph (self loop given, duplicated edge, isolated target, in-degree 10) and on the known-answer graph."""
    p = _gat_params()
    ei = A.irregular_graph(20)
    h = torch.randn(20, 22, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    for params, hh, edges in ((p, h, ei), (None, None, None)):
        if params is None:
            hh, edges, params, want_kat = parity.gat_kat_tensors()
            params = {k: v.double() for k, v in params.items()}
            hh = hh.double()
        N = hh.shape[0]
        alpha, xl, entropy, message = A.gat_attention(hh.numpy(), edges.numpy(), params)
        src, dst = A.edge_index_sl(edges.numpy(), N)
        out = np.zeros((N, 2, 11))
        np.add.at(out, dst, alpha[:, :, None] * xl[src])
        out = out.reshape(N, 22) + params[R.P_GAT + "bias"].numpy()
        want = R.gatv2_conv(hh, edges, params, 2).numpy()
        np.testing.assert_allclose(out, want, rtol=1e-13, atol=1e-14)
        sums = np.zeros((N, 2))
        np.add.at(sums, dst, alpha)
        np.testing.assert_allclose(sums, 1.0, rtol=0, atol=1e-14)
        assert (entropy >= 0).all() and (message >= 0).all()
    # the hand-computed outputs of parity.py, which holds them (and the parameters 0.3, 0.05, ...) as float32: 2^-24 * |2|
    np.testing.assert_allclose(out, want_kat.double().numpy(), rtol=0, atol=2.4e-7)
    # a graph without edges: self loops only
    alpha0, _, ent0, _ = A.gat_attention(h.numpy(), ei.numpy(), p, use_edges=False)
    assert (alpha0[-20:] == 1.0).all() and (alpha0[:-20] == 0.0).all() and (ent0 == 0.0).all()


def test_edge_pos_maps_csr_entries_to_the_given_edge_order():
    """edge_pos[q] = position of CSR entry q in edge_index with its self loops stripped, on a graph with a given self loop, a
    duplicated edge and a node with no in-edge; and the (2, E'') list rebuilt from the CSR is PyG's."""
    from tecmollm import graph
    from tecmollm.spatial_attention import edge_index_with_self_loops
    ei = A.irregular_graph(20)
    meta = graph.build(ei, 20, torch.device("cpu"), 16)
    src, dst = ei.numpy()
    keep = src != dst
    assert (~keep).sum() == 1
    s, d = src[keep], dst[keep]
    pos = meta.edge_pos.numpy()
    rowptr, colidx = meta.rowptr.numpy(), meta.colidx.numpy()
    assert pos.dtype == np.int32 and pos.shape == (meta.num_edges,) and sorted(pos.tolist()) == list(range(meta.num_edges))
    assert rowptr[8] == rowptr[7]                                            # node 7: no in-edge
    for i in range(20):
        for q in range(rowptr[i], rowptr[i + 1]):
            assert d[pos[q]] == i and s[pos[q]] == colidx[q]
        assert list(pos[rowptr[i]:rowptr[i + 1]]) == sorted(pos[rowptr[i]:rowptr[i + 1]])    # stable: given order kept
    dup = [q for q in range(rowptr[2], rowptr[3]) if colidx[q] == 1]
    assert len(dup) == 2 and pos[dup[0]] != pos[dup[1]]
    np.testing.assert_array_equal(edge_index_with_self_loops(meta).numpy(), A.edge_index_sl(ei.numpy(), 20))
    empty = graph.build(torch.zeros(2, 0, dtype=torch.int64), 3, torch.device("cpu"), 16)
    np.testing.assert_array_equal(edge_index_with_self_loops(empty).numpy(), np.stack([np.arange(3)] * 2))


def test_derived_fields_on_the_three_node_graph_by_hand():
    """parity.GAT_KAT_EDGES: edges 0 -> 1, 2 -> 1, 0 -> 2, so in PyG's order the entries are [0->1, 2->1, 0->2, 0->0, 1->1, 2->2]
    and the in-degrees (0, 2, 1).  One group, two graphs with the coefficients below (head 1 = plain averaging)."""
    from tecmollm.spatial_attention import attention_maps, derive
    ei_sl = A.edge_index_sl(np.asarray(parity.GAT_KAT_EDGES), 3)
    assert ei_sl.tolist() == [[0, 2, 0, 0, 1, 2], [1, 1, 2, 0, 1, 2]]
    unif = np.array([1 / 3, 1 / 3, 1 / 2, 1.0, 1 / 3, 1 / 2])
    g1 = np.array([0.5, 0.25, 0.75, 1.0, 0.25, 0.25])
    g2 = np.array([0.25, 0.25, 0.25, 1.0, 0.5, 0.75])
    alpha = np.stack([np.stack([g1, unif], -1), np.stack([g2, unif], -1)]).astype(np.float32)      # (2 graphs, 6, 2)
    dst = ei_sl[1]
    ent = np.stack([A.entropy_of(a, dst, 3) for a in alpha])
    msg = 2.0 * alpha
    edge, node, counts = A.accumulate_ref(alpha, msg, ent, None, 1)
    got = derive(edge, node, counts, ei_sl, 3)
    want = A.derive_ref(edge, node, counts, ei_sl, 3)
    for k in want:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-15, atol=0, err_msg=k)
    # by hand, head 0: means (0.375, 0.25, 0.5, 1, 0.375, 0.5)
    np.testing.assert_allclose(got["mean"][0, :, 0], [0.375, 0.25, 0.5, 1.0, 0.375, 0.5], rtol=1e-15)
    np.testing.assert_allclose(got["std"][0, :, 0], [0.125, 0.0, 0.25, 0.0, 0.125, 0.25], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got["message"][0, :, 0], [0.75, 0.5, 1.0, 2.0, 0.75, 1.0], rtol=1e-15)
    assert got["in_degree"].tolist() == [0, 2, 1] and got["count"].tolist() == [2.0]
    #   uniform_gap = mean - 1 / (deg_i + 1): targets (1, 1, 2, 0, 1, 2) -> 1/3, 1/3, 1/2, 1, 1/3, 1/2
    np.testing.assert_allclose(got["uniform_gap"][0, :, 0], [0.375 - 1 / 3, 0.25 - 1 / 3, 0.0, 0.0, 0.375 - 1 / 3, 0.0],
                               rtol=1e-12, atol=1e-16)
    np.testing.assert_allclose(got["uniform_gap"][0, :, 1], 0.0, atol=1e-7)          # head 1 IS plain averaging (fp32 thirds)
    #   influence: node 0 is heard by 1 (0.375) and 2 (0.5); node 2 by 1 (0.25); node 1 by nobody
    np.testing.assert_allclose(got["influence"][0, :, 0], [0.875, 0.0, 0.25], rtol=1e-15)
    np.testing.assert_allclose(got["self_weight"][0, :, 0], [1.0, 0.375, 0.5], rtol=1e-15)
    #   entropy of head 1 = ln(deg + 1), effective neighbours deg + 1
    np.testing.assert_allclose(got["effective_neighbours"][0, :, 1], [1.0, 3.0, 2.0], rtol=1e-6)
    # inflow on a line, node n at (0, n): node 1 listens to 0 (unit -1) with 0.375 and to 2 (unit +1) with 0.25; node 2 listens
    # to 0 (unit -1) with 0.5; node 0 to nobody
    maps = attention_maps(got, grid=(1, 3))
    np.testing.assert_allclose(maps["inflow_vector"][0, :, 0, 1], [0.0, -0.125, -0.5], rtol=1e-15, atol=0)
    np.testing.assert_allclose(maps["inflow_vector"][0, :, 0, 0], 0.0, atol=0)
    np.testing.assert_allclose(maps["inflow_vector"], A.inflow_ref(got["mean"], ei_sl, np.array([[0, 0], [0, 1], [0, 2.0]])),
                               rtol=1e-15, atol=0)
    coords = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 2.0]])                 # free coordinates: 0 -> 1 has unit (-0.6, -0.8)
    m2 = attention_maps(got, coords=coords)
    np.testing.assert_allclose(m2["inflow_vector"], A.inflow_ref(got["mean"], ei_sl, coords), rtol=1e-14, atol=1e-16)
    np.testing.assert_allclose(m2["inflow_vector"][0, 2, 0], [0.0, -0.5], rtol=1e-15, atol=0)


def test_a_group_without_graphs_reads_nan():
    from tecmollm.spatial_attention import attention_maps, derive
    ei_sl = A.edge_index_sl(np.asarray(parity.GAT_KAT_EDGES), 3)
    alpha = np.full((1, 6, 2), 0.5, np.float32)
    edge, node, counts = A.accumulate_ref(alpha, alpha, np.ones((1, 3, 2)), [2], 3)
    got = attention_maps(derive(edge, node, counts, ei_sl, 3), grid=(3, 1))
    assert got["count"].tolist() == [0.0, 0.0, 1.0]
    for k in ("mean", "std", "message", "uniform_gap", "self_weight", "entropy", "effective_neighbours", "influence",
              "inflow_vector"):
        assert np.isnan(got[k][:2]).all() and np.isfinite(got[k][2]).all(), k


def test_abi_declares_binds_and_exports_the_two_entries():
    from tecmollm import _lib, ops
    import tecmollm
    header = open(os.path.join(ROOT, "include", "tecmollm.h")).read()
    assert "int64_t tecm_spatial_attention_ws_floats(const TecmSpatial* d, const TecmSpatialAttn* a);" in header
    assert "int tecm_spatial_attention(const TecmSpatial* d, const TecmSpatialAttn* a, void* stream);" in header
    assert "#define TECM_ATTN_SKIP_UNCONNECTED 1" in header and _lib.TECM_ATTN_SKIP_UNCONNECTED == 1
    assert int(re.search(r"#define\s+TECM_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION == 21
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tecm_spatial_attention_ws_floats", "tecm_spatial_attention"):
        assert name in _lib.EXPORTS and hasattr(handle, name)
    body = re.search(r"typedef struct TecmSpatialAttn \{(.*?)\} TecmSpatialAttn;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*[;]", body)
    assert names == [f[0] for f in _lib.TecmSpatialAttn._fields_]
    assert ctypes.sizeof(_lib.TecmSpatialAttn) == 8 * 8 + 4 * 4
    assert _lib.lib().tecm_abi_version() == 21
    # pure host arithmetic: 48 floats per row, and 2 (E'' * 2) + 2 N more per graph when accumulating; 64 MiB chunks
    d = _lib.TecmSpatial(B=16, L=48, N=2911, Cin=6, Demb=16, H=2, graphs_with_edges=768, num_tiles=27, tile_nodes=110,
                         win_max=256, tile_edges_max=1110, year_rows=13, out_ld=24)
    for f in ("x", "tf", "node_tab", "tod_tab", "doy_tab", "year_tab", "season_tab", "Wl", "bl", "Wr", "br", "att", "bias",
              "rowptr", "colidx", "tile_lo", "tile_hi", "err_flag"):
        setattr(d, f, 64)                                                   # never dereferenced on the host
    E1 = 28000
    per_graph = 2911 * 48
    assert ops.spatial_attention_ws_floats(d, E1, False) == ((64 << 20) // (4 * per_graph)) * per_graph
    per_graph_acc = per_graph + 4 * (E1 + 2911) + 2 * 2911
    assert ops.spatial_attention_ws_floats(d, E1, True) == ((64 << 20) // (4 * per_graph_acc)) * per_graph_acc
    d.B, d.L = 1, 2
    assert ops.spatial_attention_ws_floats(d, E1, False) == 2 * per_graph
    d.Cin, d.Demb, d.flags = 22, 0, 2
    assert ops.spatial_attention_ws_floats(d, E1, False) == 2 * per_graph   # the stand-alone GATv2
    d.flags = 0
    assert ops.spatial_attention_ws_floats(d, E1, False) == 0               # 22 input channels without NO_RESIDUAL: not served
    d.Cin, d.Demb = 8, 14
    assert ops.spatial_attention_ws_floats(d, E1, False) == 0
    a = _lib.TecmSpatialAttn(E=E1)
    assert _lib.lib().tecm_spatial_attention(ctypes.byref(d), ctypes.byref(a), None) == -1    # TECM_E_ARG before any launch
    assert _lib.lib().tecm_spatial_attention(None, None, None) == -1
    for name in ("spatial_attention", "AttentionStats", "evaluate_attention", "attention_maps", "write_attention",
                 "graph_groups_by_sample", "graph_groups_by_slot", "graph_groups_by_lag"):
        assert callable(getattr(tecmollm, name)) and name in tecmollm.__all__


def test_cpu_tensors_are_refused():
    import pytest
    from tecmollm import TecmError, spatial_attention

    class Stub:
        pass
    with pytest.raises(TecmError):
        spatial_attention(Stub(), torch.zeros(1, 2, 3, 6), torch.zeros(1, 2, 3, 4), torch.zeros(2, 0, dtype=torch.int64))


def test_write_attention_writes_the_stated_files(tmp_path):
    from tecmollm.spatial_attention import derive, write_attention
    rows, cols, G = 2, 3, 2
    N = rows * cols
    ei = R.grid_graph(rows, cols, threshold_km=170.0)[0].numpy()
    ei_sl = A.edge_index_sl(ei, N)
    E2 = ei_sl.shape[1]
    rng = np.random.default_rng(0)
    alpha = rng.random((5, E2, 2)).astype(np.float32)
    ent = rng.random((5, N, 2))
    edge, node, counts = A.accumulate_ref(alpha, 3 * alpha, ent, [0, 1, 1, 0, 1], G)
    att = derive(edge, node, counts, ei_sl, N)
    att["edge_index_sl"] = ei_sl
    paths = write_attention(att, str(tmp_path), grid=(rows, cols))
    assert sorted(os.path.basename(p) for p in paths.values()) == ["attention_by_group.csv", "attention_maps.npz"]
    z = np.load(paths["npz"])
    assert set(z.files) == {"count", "edge_index_sl", "in_degree", "self_weight", "entropy", "effective_neighbours",
                            "influence", "inflow_vector", "mean", "std", "message", "uniform_gap"}
    for k in ("self_weight", "entropy", "effective_neighbours", "influence"):
        assert z[k].shape == (G, 2, rows, cols)
        np.testing.assert_array_equal(z[k][1, 0].reshape(-1), att[k][1, :, 0])
    assert z["inflow_vector"].shape == (G, 2, rows, cols, 2) and z["in_degree"].shape == (rows, cols)
    for k in ("mean", "std", "message", "uniform_gap"):
        assert z[k].shape == (G, E2, 2)
    assert z["edge_index_sl"].shape == (2, E2) and z["count"].tolist() == [2.0, 3.0]
    lines = open(paths["csv"]).read().strip().splitlines()
    assert lines[0] == "group,head,count,self_weight_mean,effective_neighbours_mean,abs_uniform_gap_mean"
    assert len(lines) == 1 + G * 2 and lines[3].startswith("1,0,3,")
    assert float(lines[3].split(",")[3]) == float(np.mean(att["self_weight"][1, :, 0]))
