"""CPU tests of the host side of the input gradient: the whole-graph by-source CSR that csrc/spatial_dx.hip sweeps, against a
brute-force construction; the attribution maps and their files."""
import csv
import os

import numpy as np
import pytest
import torch

from tests.input_grad_cases import (GRID_ONE_TILE, GRID_TWO_TILES, GRID_WIDE, NO_IN, NO_OUT, asymmetric_edges,
                                    brute_by_source, grid_edges)


def _graphs():
    return {"one_tile": (grid_edges(GRID_ONE_TILE), 12), "two_tiles": (grid_edges(GRID_TWO_TILES), 135),
            "asymmetric": (asymmetric_edges(), 135), "empty": (torch.zeros(2, 0, dtype=torch.int64), 5),
            "loops_only": (torch.tensor([[0, 2], [0, 2]]), 3)}


@pytest.mark.parametrize("name", ["one_tile", "two_tiles", "asymmetric", "empty", "loops_only"])
def test_by_source_csr_matches_brute_force_and_slots_are_by_target_positions(name):
    from tecmollm import graph as G
    ei, N = _graphs()[name]
    rowptr, colidx = G.csr_by_target(ei.numpy(), N)
    ptr, tgt, slot = G.csr_by_source(rowptr, colidx, N)
    bptr, btgt, bslot = brute_by_source(ei.numpy(), N)
    assert ptr.dtype == tgt.dtype == slot.dtype == np.int32
    assert np.array_equal(ptr, bptr) and np.array_equal(tgt, btgt) and np.array_equal(slot, bslot)
    # every entry names its own position in the target's list: the forward's dropout index is ((row*H + head)*ld + slot)
    src = np.repeat(np.arange(N), np.diff(ptr))
    assert np.array_equal(colidx[rowptr[tgt] + slot], src)
    assert ((slot >= 0) & (slot < np.diff(rowptr)[tgt])).all()
    assert len(set(zip(tgt.tolist(), slot.tolist()))) == colidx.size      # a permutation of the by-target entries


def test_asymmetric_graph_is_what_its_name_says():
    from tecmollm import graph as G
    ei = asymmetric_edges()
    rowptr, colidx = G.csr_by_target(ei.numpy(), 135)
    ptr, tgt, _ = G.csr_by_source(rowptr, colidx, 135)
    assert rowptr[NO_IN + 1] == rowptr[NO_IN] and ptr[NO_IN + 1] > ptr[NO_IN]
    assert ptr[NO_OUT + 1] == ptr[NO_OUT] and rowptr[NO_OUT + 1] > rowptr[NO_OUT]
    assert int((ei[0] == ei[1]).sum()) == 5
    pairs = set(zip(ei[0].tolist(), ei[1].tolist()))
    assert sum((i, j) not in pairs for j, i in pairs if i != j) > 50       # direction matters


def test_graph_meta_carries_the_by_source_csr_and_keeps_its_tiling():
    """graph.build: the new fields next to the old ones, device pointers never null (one zero entry in an empty graph); the
    windows the GPU tests rely on."""
    from tecmollm import graph as G
    for grid, want in ((GRID_ONE_TILE, (128, 1, 12)), (GRID_TWO_TILES, (128, 2, 135)), (GRID_WIDE, (64, 7, 346))):
        N = grid[0] * grid[1]
        meta = G.build(grid_edges(grid), N, torch.device("cpu"))
        assert (meta.tile_nodes, meta.num_tiles, meta.win_max) == want
        rowptr, colidx = G.csr_by_target(grid_edges(grid).numpy(), N)
        ptr, tgt, slot = G.csr_by_source(rowptr, colidx, N)
        assert torch.equal(meta.out_ptr, torch.from_numpy(ptr)) and torch.equal(meta.out_target, torch.from_numpy(tgt))
        assert torch.equal(meta.out_slot, torch.from_numpy(slot))
        assert meta.out_ptr.dtype == meta.out_target.dtype == meta.out_slot.dtype == torch.int32
    assert 256 < G.build(grid_edges(GRID_WIDE), 420, torch.device("cpu")).win_max <= G.MAX_WINDOW
    empty = G.build(torch.zeros(2, 0, dtype=torch.int64), 5, torch.device("cpu"))
    assert empty.out_ptr.tolist() == [0] * 6 and empty.out_target.numel() == 1 and empty.out_slot.numel() == 1


def test_library_reports_the_input_gradient_workspace_and_refuses_what_it_does_not_serve(monkeypatch):
    """tecm_spatial_dx_ws_floats is pure host arithmetic: 56 floats per row of a chunk of graphs (x_l, x_r, statistics), a
    chunk of at most 64 MiB; 0 for the stand-alone encoder (flags, Demb = 0).  tecm_spatial_dx refuses before any launch."""
    import ctypes as C
    from tecmollm import _lib
    h = _lib.lib()
    monkeypatch.delenv("TECM_SPATIAL_DX_GRAPHS", raising=False)
    live = (C.c_float * 4)()
    d = _lib.TecmSpatial()
    d.B, d.L, d.N, d.Cin, d.Demb, d.H = 8, 48, 2911, 6, 16, 2
    d.graphs_with_edges, d.num_tiles, d.tile_nodes, d.win_max, d.tile_edges_max, d.year_rows = 1, 26, 112, 256, 1110, 13
    for name in ("x", "tf", "node_tab", "tod_tab", "doy_tab", "year_tab", "season_tab", "Wl", "bl", "Wr", "br", "att", "bias",
                 "rowptr", "colidx", "tile_lo", "tile_hi", "err_flag"):
        setattr(d, name, C.addressof(live))
    d.flags, d.out_ld = 0, 24
    per_chunk = (64 << 20) // (2911 * 56 * 4)
    assert per_chunk == 102 and h.tecm_spatial_dx_ws_floats(C.byref(d)) == per_chunk * 2911 * 56
    d.B, d.L = 1, 16
    assert h.tecm_spatial_dx_ws_floats(C.byref(d)) == 16 * 2911 * 56
    monkeypatch.setenv("TECM_SPATIAL_DX_GRAPHS", "3")
    assert h.tecm_spatial_dx_ws_floats(C.byref(d)) == 3 * 2911 * 56
    d.flags = 2
    assert h.tecm_spatial_dx_ws_floats(C.byref(d)) == 0
    g = _lib.TecmSpatialDx()
    assert h.tecm_spatial_dx(C.byref(d), C.byref(g), None) == -1                    # TECM_E_ARG
    assert b"flags" in h.tecm_last_error()
    d.flags, d.Cin, d.Demb = 0, 22, 0
    assert h.tecm_spatial_dx_ws_floats(C.byref(d)) == 0
    d.Cin, d.Demb = 10, 12
    assert h.tecm_spatial_dx(C.byref(d), C.byref(g), None) == -1                    # TECM_E_ARG: null pointers in TecmSpatialDx
    assert b"null pointer" in h.tecm_last_error()


def test_attribution_maps_on_a_hand_made_tensor():
    from tecmollm import attribution_maps
    attr = torch.zeros(2, 3, 4, 2)                         # (B, L, N, C)
    attr[0, 0, 1, 0], attr[0, 2, 1, 0], attr[1, 0, 3, 0] = 2.0, -4.0, 6.0
    attr[0, 1, 2, 1], attr[1, 1, 2, 1] = -1.0, 3.0
    m = attribution_maps(attr, ["tec", "kp"])
    assert m["channel_names"] == ["tec", "kp"]
    lag = torch.tensor([[4.0, 0.0], [0.0, 2.0], [2.0, 0.0]])
    node = torch.tensor([[0.0, 0.0], [3.0, 0.0], [0.0, 2.0], [3.0, 0.0]])
    assert torch.equal(m["lag_channel"], lag) and torch.equal(m["node_channel"], node)
    assert torch.equal(m["channel"], torch.tensor([6.0, 2.0]))
    assert attribution_maps(attr)["channel_names"] == ["channel0", "channel1"]
    with pytest.raises(ValueError):
        attribution_maps(attr, ["only one"])
    with pytest.raises(ValueError):
        attribution_maps(attr[0])


def test_write_attributions_round_trip(tmp_path):
    from tecmollm import attribution_maps, write_attributions
    attr = torch.randn(3, 5, 6, 4, generator=torch.Generator().manual_seed(1))
    m = attribution_maps(attr, ["tec", "f107", "kp", "ap"])
    paths = write_attributions(m, str(tmp_path / "flat"))
    z = np.load(paths["npz"])
    assert sorted(z.files) == ["channel", "lag_channel", "node_channel"]
    for k in z.files:
        assert np.array_equal(z[k], m[k].numpy())
    rows = list(csv.reader(open(paths["csv"], newline="", encoding="utf-8")))
    assert rows[0] == ["channel", "attribution", "share"] and [r[0] for r in rows[1:]] == m["channel_names"]
    assert [float(r[1]) for r in rows[1:]] == [float(v) for v in m["channel"]]
    assert abs(sum(float(r[2]) for r in rows[1:]) - 1.0) < 1e-6
    on_grid = np.load(write_attributions(m, str(tmp_path / "grid"), grid=(2, 3))["npz"])
    assert on_grid["node_channel"].shape == (2, 3, 4)
    assert np.array_equal(on_grid["node_channel"].reshape(6, 4), m["node_channel"].numpy())
    with pytest.raises(ValueError, match="does not hold 6 nodes"):
        write_attributions(m, str(tmp_path / "bad"), grid=(2, 2))
    assert os.path.basename(paths["npz"]) == "attributions.npz" and os.path.basename(paths["csv"]) == "attribution_by_channel.csv"
