"""CPU tests of the per-cell evaluation metrics' host side: the vectorised derivation against `HorizonMetrics.compute()` and
against the reference's own `evaluate_metrics` (tools/make_golden_error_maps.py), the window grouping rule, the map
files, the rank merge of the statistics (two gloo ranks) and the entry point's presence in the C ABI."""
import csv
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.error_maps_ref import accumulate, pipeline, terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg", "mae_by_horizon", "rmse_by_horizon", "r2_by_horizon",
        "pearson_by_horizon")
MAP_KEYS = ("count", "mae", "rmse", "bias", "r2_score", "pearson_r")


def _rows():
    """(5, 8) statistics of hand-made series: ordinary, constant target, constant prediction, perfect, another ordinary."""
    rng = np.random.default_rng(4)
    t = rng.gamma(2.0, 12.0, size=(5, 200)).astype(np.float32)
    p = (t + rng.standard_normal((5, 200)) * 3).astype(np.float32)
    t[1] = np.float32(17.3)                                                # constant target
    p[2] = np.float32(41.7)                                                # constant prediction
    p[3] = t[3]                                                            # perfect
    return terms(t, p).sum(axis=2).T, t, p


def test_derive_reproduces_horizon_metrics_compute_row_by_row():
    from src.evaluation.metrics import HorizonMetrics, derive
    rows, t, p = _rows()
    hm = HorizonMetrics(5, None, device="cpu")
    hm.stats.copy_(torch.from_numpy(rows))
    want = hm.compute()
    got = derive(rows)
    assert set(got) == set(MAP_KEYS)
    for name, key in (("mae", "mae_by_horizon"), ("rmse", "rmse_by_horizon"), ("r2_score", "r2_by_horizon"),
                      ("pearson_r", "pearson_by_horizon")):
        assert got[name].shape == (5,)
        assert got[name].tolist() == want[key], name                       # the same operations: the same bits
    assert got["r2_score"][1] == 0.0 and got["pearson_r"][1] == 0.0        # constant target, imperfect forecast
    assert got["pearson_r"][2] == 0.0 and got["r2_score"][2] < 0           # constant prediction
    assert got["r2_score"][3] == 1.0 and got["mae"][3] == 0.0 and got["pearson_r"][3] == pytest.approx(1.0, abs=1e-12)
    assert got["count"].tolist() == [200.0] * 5
    np.testing.assert_allclose(got["bias"], (p.astype(np.float64) - t).mean(axis=1), rtol=1e-12, atol=1e-12)
    # leading axes are free, and a cell without samples reads NaN instead of raising
    grid = np.zeros((2, 5, 3, 8))
    grid[0, :, 1] = rows
    out = derive(grid)
    for k in MAP_KEYS[1:]:
        assert out[k].shape == (2, 5, 3)
        assert np.array_equal(out[k][0, :, 1], got[k]) and np.isnan(out[k][1]).all() and np.isnan(out[k][0, :, 0]).all()
    assert out["count"][1].sum() == 0


def test_derive_matches_the_reference_cell_by_cell(golden_dir):
    """The reference's evaluate_horizons / evaluate_metrics run on every (horizon, node) cell of a 40 x 3 x 5 problem with a
    fitted scaler, a NaN and a +inf prediction, a constant node and predictions clipped at both ends.  rtol 2e-5: the
    reference sums in float32 (the bar of tests/test_gpu_shell.py for the same comparison)."""
    from src.evaluation.metrics import derive
    g = np.load(os.path.join(golden_dir, "error_maps.npz"))
    S, H, I = g["y_true"].shape
    assert (S, H, I) == (40, 3, 5) and np.isnan(g["y_pred"]).sum() == 1 and np.isposinf(g["y_pred"]).sum() == 1
    stats, mags = np.zeros((1, H, 8, I)), np.zeros((1, H, 8, I))
    accumulate(stats, mags, g["y_pred"], g["y_true"], None, (float(g["mean"]), float(g["scale"])))
    got = derive(stats[0].transpose(0, 2, 1))
    t, p = pipeline(g["y_pred"], g["y_true"], (float(g["mean"]), float(g["scale"])))
    assert p.min() == 0.0 and p.max() == 200.0                             # both ends of the clip are hit
    for k in ("mae", "rmse", "r2_score", "pearson_r"):
        np.testing.assert_allclose(got[k], g[f"out_{k}"], rtol=2e-5, atol=0, err_msg=k)
    c = int(g["constant_node"])
    assert (got["r2_score"][:, c] == 0).all() and (got["pearson_r"][:, c] == 0).all()


def _loop_groups(series, starts, L_in, L_out, edges, span, reduce):
    out = []
    for a in starts:
        win = series[a:a + L_in] if span == "input" else series[a + L_in:a + L_in + L_out]
        v = {"max": max(win), "min": min(win), "last": win[-1]}[reduce]
        out.append((sum(1 for e in edges if e < v), v))                   # an edge that equals the value is not below it
    return [g for g, _ in out], [v for _, v in out]


@pytest.mark.parametrize("span", ["input", "target"])
@pytest.mark.parametrize("reduce", ["max", "min", "last"])
def test_window_group_rule_matches_a_plain_loop(span, reduce):
    from tecmollm.evaluate import _window_groups
    series = np.round(4 + 3.9 * np.sin(np.arange(60) / 5.0)).astype(np.float32)   # Kp-like: whole numbers, so edges hit values
    L_in, L_out, stride = 7, 4, 3
    starts = list(range(0, 60 - L_in - L_out + 1, stride))
    edges = [2.0, 4.0, 6.0]
    got = _window_groups(torch.from_numpy(series), torch.tensor(starts), L_in, L_out, edges, span, reduce)
    want, values = _loop_groups(series.tolist(), starts, L_in, L_out, edges, span, reduce)
    assert got.dtype == torch.int32 and got.tolist() == want
    assert len(set(want)) > 1 and set(values) & set(edges)                # several groups, and values that sit on an edge
    # undoing a feature scaling first: the same groups from the scaled series
    scaled = torch.from_numpy((series - 3.5) / 2.0)
    assert _window_groups(scaled, torch.tensor(starts), L_in, L_out, edges, span, reduce, 3.5, 2.0).tolist() == want
    with pytest.raises(ValueError):
        _window_groups(scaled, torch.tensor(starts), L_in, L_out, edges, "both", reduce)
    with pytest.raises(ValueError):
        _window_groups(scaled, torch.tensor(starts), L_in, L_out, edges, span, "mean")


def _maps(G=2, H=3, I=6):
    from src.evaluation.metrics import _pooled, derive
    rng = np.random.default_rng(2)
    out = {}
    for name in ("TEC-MoLLM", "HistoricalAverage"):
        t = rng.gamma(2.0, 12.0, size=(G, H, I, 30)).astype(np.float32)
        p = (t + rng.standard_normal(t.shape)).astype(np.float32)
        st = np.moveaxis(terms(t, p).sum(axis=-1), 0, -1)                  # (G, H, I, 8)
        st[1] = 0                                                          # a group the split never visits
        m = dict(derive(st))
        m["by_group"] = [_pooled(derive(st[g].sum(axis=1))) for g in range(G)]
        out[name] = m
    return out


@pytest.mark.parametrize("grid", [None, (2, 3)])
def test_write_maps_round_trips(tmp_path, grid):
    from tecmollm.evaluate import write_maps
    maps = _maps()
    paths = write_maps(maps, str(tmp_path / "out"), grid=grid)
    assert sorted(os.listdir(tmp_path / "out")) == ["error_maps.npz", "evaluation_by_group.csv"]
    z = np.load(paths["npz"])
    assert sorted(z.files) == sorted(f"{n}/{k}" for n in maps for k in MAP_KEYS)
    for n in maps:
        for k in MAP_KEYS:
            a = z[f"{n}/{k}"]
            assert a.shape == ((2, 3, 6) if grid is None else (2, 3, 2, 3))
            assert np.array_equal(a.reshape(2, 3, 6), maps[n][k], equal_nan=True)
    with open(paths["csv"], newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["forecast", "group", "count", "mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg"]
    assert [(r[0], r[1]) for r in rows[1:]] == [(n, str(g)) for n in maps for g in range(2)]
    for r in rows[1:]:
        pooled = maps[r[0]]["by_group"][int(r[1])]
        assert int(r[2]) == (6 * 30 if r[1] == "0" else 0)
        for cell, k in zip(r[3:], KEYS[:4]):
            assert float(cell) == pooled[k] or (np.isnan(float(cell)) and np.isnan(pooled[k]))
    assert set(maps["TEC-MoLLM"]["by_group"][0]) == set(KEYS)
    with pytest.raises(ValueError):
        write_maps(maps, str(tmp_path / "bad"), grid=(4, 2))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_stats(rank):
    g = torch.Generator().manual_seed(300 + rank)
    return torch.rand(3, 4, 8, 7, generator=g, dtype=torch.float64) * 1e6 + rank


def _merge_worker(rank, port, out_dir):
    import sys
    for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from src.evaluation.metrics import MapMetrics
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    try:
        mm = MapMetrics(4, 7, 3, None, device="cpu")
        assert mm.stats.shape == (3, 4, 8, 7)
        mm.stats.copy_(_rank_stats(rank))
        assert mm.merge_() is mm
        mm2 = MapMetrics(4, 7, 3, None, device="cpu")
        mm2.stats.copy_(_rank_stats(rank))
        mm2.merge_(dist.new_group([0, 1]))
        torch.save({"merged": mm.stats, "merged_group": mm2.stats}, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_map_merge_on_two_gloo_ranks_is_the_plain_sum(tmp_path):
    mp.spawn(_merge_worker, args=(_free_port(), str(tmp_path)), nprocs=2, join=True)
    want = _rank_stats(0) + _rank_stats(1)
    for rank in (0, 1):
        got = torch.load(os.path.join(tmp_path, f"rank{rank}.pt"))
        assert torch.equal(got["merged"], want) and torch.equal(got["merged_group"], want)     # exactly


def test_map_metrics_host_side_without_a_process_group():
    from src.evaluation.metrics import HorizonMetrics, MapMetrics
    assert not dist.is_initialized()
    mm = MapMetrics(4, 7, 3, (20.0, 8.0), device="cpu")
    mm.stats.copy_(_rank_stats(0))
    assert mm.merge_() is mm and torch.equal(mm.stats, _rank_stats(0))
    np.testing.assert_allclose(mm.collapse(), _rank_stats(0).sum(dim=(0, 3)).numpy(), rtol=1e-15)
    out = mm.compute()
    assert set(out) == set(MAP_KEYS) | {"by_group"} and len(out["by_group"]) == 3
    hm = HorizonMetrics(4, None, device="cpu")                             # a group's pooled dict is HorizonMetrics' own
    hm.stats.copy_(_rank_stats(0)[1].sum(dim=2))
    want = hm.compute()
    assert set(out["by_group"][1]) == set(want)
    for k in KEYS:
        np.testing.assert_allclose(np.asarray(out["by_group"][1][k]), np.asarray(want[k]), rtol=1e-12, err_msg=k)
    mm.reset()
    assert float(mm.stats.abs().sum()) == 0.0 and np.isnan(mm.compute()["mae"]).all()
    with pytest.raises(ValueError):
        MapMetrics(4, 0)


def test_metrics_map_is_exported_and_refuses_a_null_descriptor():
    from tecmollm import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "tecm_metrics_map")
    assert _lib.ABI_VERSION == 21 and _lib.lib().tecm_abi_version() == 21
    assert _lib.lib().tecm_metrics_map(None, None) == -1                   # TECM_E_ARG, before any device call
    assert b"null descriptor" in _lib.lib().tecm_last_error()
    m = _lib.TecmMetricsMap()                                             # all pointers null
    assert _lib.lib().tecm_metrics_map(ctypes.byref(m), None) == -1
    header = open(os.path.join(ROOT, "include", "tecmollm.h")).read()
    assert "#define TECM_BAD_GROUP 16" in header
    from tecmollm import devcheck
    assert devcheck.BAD_GROUP == 16 and _lib.TECM_MAP_LDS_MAX_H == 32 and "#define TECM_MAP_LDS_MAX_H 32" in header
