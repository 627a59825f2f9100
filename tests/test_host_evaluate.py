"""CPU tests of the evaluation layer's host side: the improvement percentages, the report files, the hour-to-slot rule and
the rank merge of the metric statistics (two gloo ranks)."""
import csv
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

KEYS = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg", "mae_by_horizon", "rmse_by_horizon", "r2_by_horizon",
        "pearson_by_horizon")


def _results():
    def entry(mae, rmse, r2, pear):
        return {"mae_avg": mae, "rmse_avg": rmse, "r2_score_avg": r2, "pearson_r_avg": pear,
                "mae_by_horizon": [mae - 0.5, mae + 0.5], "rmse_by_horizon": [rmse - 0.25, rmse + 0.25],
                "r2_by_horizon": [r2 + 0.125, r2 - 0.125], "pearson_by_horizon": [pear, pear]}
    return {"TEC-MoLLM": entry(2.0, 3.0, 0.75, 0.9), "HistoricalAverage": entry(8.0, 12.0, -0.5, 0.6),
            "Persistence": entry(4.0, 4.0, 0.25, 0.75)}


def test_improvement_percentages_including_a_negative_baseline_r2():
    """test.py:243-251 by hand: (8 - 2) / 8, (12 - 3) / 12, (0.75 - -0.5) / |-0.5|, (0.9 - 0.6) / 0.6."""
    from tecmollm.evaluate import improvement
    got = improvement(_results())
    assert set(got) == {"mae", "rmse", "r2_score", "pearson_r"}
    assert got["mae"] == pytest.approx(75.0, rel=1e-15) and got["rmse"] == pytest.approx(75.0, rel=1e-15)
    assert got["r2_score"] == pytest.approx(250.0, rel=1e-15)             # positive although the baseline's R^2 is negative
    assert got["pearson_r"] == pytest.approx(50.0, rel=1e-14)
    other = improvement(_results(), baseline="Persistence")
    assert other["mae"] == pytest.approx(50.0) and other["rmse"] == pytest.approx(25.0)
    assert other["r2_score"] == pytest.approx(200.0) and other["pearson_r"] == pytest.approx(20.0)
    worse = improvement(_results(), model="HistoricalAverage", baseline="TEC-MoLLM")
    assert worse["mae"] == pytest.approx(-300.0) and worse["r2_score"] == pytest.approx(-125.0 / 0.75)


def test_write_report_files_parse_back(tmp_path):
    from tecmollm.evaluate import write_report
    res = _results()
    res["TEC-MoLLM"]["mae_avg"] = np.float64(2.0)                          # numpy scalars must not leak their repr
    res["TEC-MoLLM"]["mae_by_horizon"] = [np.float64(1.5), np.float64(2.5)]
    paths = write_report(res, str(tmp_path / "results"))
    assert sorted(os.listdir(tmp_path / "results")) == ["evaluation_results.csv", "evaluation_summary.txt"]
    with open(paths["csv"], newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    assert rows[0] == [""] + list(KEYS)                                    # first header cell empty, one column per key
    assert [r[0] for r in rows[1:]] == ["TEC-MoLLM", "HistoricalAverage", "Persistence"]
    want = _results()
    for r in rows[1:]:
        for k, cell in zip(KEYS, r[1:]):
            v = want[r[0]][k]
            if isinstance(v, list):
                assert cell == repr(v) and cell.startswith("[")             # list-valued cells as their repr
                assert [float(x) for x in cell.strip("[]").split(",")] == v
            else:
                assert float(cell) == v
    text = open(paths["summary"], encoding="utf-8").read()
    blocks = [b for b in text.split("\n\n") if ":" in b and not b.startswith("TEC-MoLLM evaluation")]
    blocks = {b.splitlines()[0].rstrip(":"): b.splitlines()[1:] for b in blocks}
    assert list(blocks) == ["TEC-MoLLM", "HistoricalAverage", "Persistence"]
    for name, lines in blocks.items():
        nums = [ln.rsplit(" ", 1)[1] for ln in lines]
        assert nums == [f"{want[name][k]:.6f}" for k in KEYS[:4]]           # the four averages, six decimals
    assert "-0.500000" in text


def test_time_slots_rule_matches_the_reference(golden_dir):
    """`datetime64[h] % 24 // 2` against slots read off the reference's own predict (tools/make_golden_evaluate.py)."""
    from src.models.baselines import time_slots
    g = np.load(os.path.join(golden_dir, "evaluate_historical_average.npz"))
    assert np.array_equal(time_slots(g["when"].astype("datetime64[h]")), g["when_slots"])
    assert np.array_equal(time_slots(g["when"]), g["when_slots"])          # integers count hours
    assert np.array_equal(time_slots(torch.from_numpy(g["when"])), g["when_slots"])
    fine = g["when"].astype("datetime64[h]").astype("datetime64[s]") + np.timedelta64(59 * 60 + 59, "s")
    assert np.array_equal(time_slots(fine), g["when_slots"])              # finer units truncate to the hour
    assert np.array_equal(time_slots(g["hours"][:24]), np.arange(24) % 12)  # the 2-hourly fit stamps: one slot per step
    day = np.datetime64("2020-02-29T00", "h") + np.arange(24).astype("timedelta64[h]")
    assert time_slots(day).tolist() == [h // 2 for h in range(24)]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _merge_worker(rank, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tec-mollm_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from src.evaluation.metrics import HorizonMetrics
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    try:
        hm = HorizonMetrics(5, None, device="cpu")
        hm.stats.copy_(_rank_stats(rank))
        assert hm.merge_() is hm
        sub = dist.new_group([0, 1])
        hm2 = HorizonMetrics(5, None, device="cpu")
        hm2.stats.copy_(_rank_stats(rank))
        hm2.merge_(sub)
        torch.save({"merged": hm.stats, "merged_group": hm2.stats}, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _rank_stats(rank):
    g = torch.Generator().manual_seed(100 + rank)
    return torch.rand(5, 8, generator=g, dtype=torch.float64) * 1e6 + rank


def test_merge_on_two_gloo_ranks_is_the_plain_sum(tmp_path):
    mp.spawn(_merge_worker, args=(_free_port(), str(tmp_path)), nprocs=2, join=True)
    want = _rank_stats(0) + _rank_stats(1)
    for rank in (0, 1):
        got = torch.load(os.path.join(tmp_path, f"rank{rank}.pt"))
        assert torch.equal(got["merged"], want) and torch.equal(got["merged_group"], want)     # exactly


def test_merge_without_a_process_group_is_a_no_op():
    from src.evaluation.metrics import HorizonMetrics
    assert not dist.is_initialized()
    hm = HorizonMetrics(5, (20.0, 8.0), device="cpu")
    hm.stats.copy_(_rank_stats(0))
    assert hm.merge_() is hm and torch.equal(hm.stats, _rank_stats(0))


def test_validate_and_evaluate_split_take_order_and_group():
    import inspect
    from tecmollm.evaluate import evaluate_split
    from tecmollm.loop import validate
    p = inspect.signature(validate).parameters
    assert p["order"].kind is p["group"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["order"].default is None and p["group"].default is None
    assert list(p)[:6] == ["model", "dataset", "edge_index", "batch_size", "scaler", "edge_weight"]
    q = inspect.signature(evaluate_split).parameters
    assert list(q) == ["model", "dataset", "edge_index", "batch_size", "scaler", "baselines", "edge_weight", "order", "group"]
    assert q["baselines"].default == ("mean",)
