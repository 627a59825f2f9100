"""GPU tests of the significance feature: the per-window statistics (tecm_metrics_window) against the ordered float64
restatement and against `HorizonMetrics`, the paired circular block bootstrap (tecm_block_bootstrap) bit for bit against
the sequential restatement (tests/significance_ref.py), its coverage on autocorrelated series, and score / resample / test /
write end to end on a tiny model.

Bars: the bootstrap only adds, so it is exact.  The per-window sums are held to the error maps' bar
(tests/test_gpu_error_maps.py): |kernel - numpy| <= 1e-12 * sum |terms|, both sides adding the same float64 terms in the same
order, so only FMA contraction inside a term lies between them; the counts are exact."""
import math
import os

import numpy as np
import pytest
import torch

from tests import significance_ref as SR

pytestmark = pytest.mark.gpu

BAR = 1e-12
SCALER = (21.5, 9.25)
SENTINEL = -777.0
LAYOUTS = ("model", "contiguous", "baseline", "strided")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


# ------------------------------------------------------------------------------------ per-window statistics
def _hard(S, H, I, rng):
    """Scaled forecasts and truths with NaN and both infinities in both, and values far outside the clip range."""
    p = (rng.standard_normal((S, H, I)) * 2.5).astype(np.float32)
    t = (rng.standard_normal((S, H, I)) * 2.5).astype(np.float32)
    p[rng.random(p.shape) < 0.1] = np.float32(-30.0)
    p[rng.random(p.shape) < 0.05] = np.float32(+40.0)
    for a in (p.reshape(-1), t.reshape(-1)):
        if a.size >= 6:
            w = rng.choice(a.size, size=3, replace=False)
            a[w[0]], a[w[1]], a[w[2]] = np.nan, np.inf, -np.inf
    return p, t


def _layout(a, layout, dev):
    """(S, H, I) numpy -> (device view, the numpy array it holds).  model: stride_h = 1, stride_i = H (the permuted output);
    baseline: horizon 0 expanded with stride_h = 0; strided: every other element of a wider row, rows padded."""
    if layout == "baseline":
        a = np.ascontiguousarray(np.broadcast_to(a[:, :1], a.shape))
        return torch.from_numpy(a[:, 0]).to(dev).unsqueeze(1).expand(*a.shape), a
    d = torch.from_numpy(a).to(dev)
    if layout == "model":
        d = d.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    elif layout == "strided":
        wide = torch.full((a.shape[0], a.shape[1] + 1, 2 * a.shape[2] + 3), 1e30, device=dev)
        wide[:, :a.shape[1], 1:1 + 2 * a.shape[2]:2] = d
        d = wide[:, :a.shape[1], 1:1 + 2 * a.shape[2]:2]
    return d, a


def _assert_table(got, want, mags, what):
    assert np.array_equal(got[..., 0], want[..., 0]), what                 # the counts exactly
    assert np.isfinite(want).all(), what
    err = np.abs(got - want)
    worst = float(np.max(err / np.maximum(mags, 1e-300)))
    print(f"{what}: max |kernel - numpy| / sum|terms| = {worst:.3e}")
    assert np.all(err <= BAR * mags), (what, worst)


@pytest.mark.parametrize("H", [1, 12, 24, 50])
@pytest.mark.parametrize("I", [1, 63, 64, 65, 135])
def test_window_statistics_match_the_ordered_restatement(dev, I, H):
    """S = 5 (and S = 1) x four layouts of the forecast x scaler + clip on / off, hard values in both operands, rows
    scattered and non-monotone into a larger table whose other rows hold a sentinel; a second update of the same rows
    replaces the first."""
    from tecmollm.devcheck import check_device_errors
    from tecmollm.significance import window_stats
    rng = np.random.default_rng(1000 * I + H)
    for S, rows in ((1, [4]), (5, [6, 0, 3, 8, 1])):
        p, t = _hard(S, H, I, rng)
        first = _hard(S, H, I, rng)
        td = torch.from_numpy(t).to(dev)
        rows_d = torch.tensor(rows, dtype=torch.int64, device=dev)
        others = [r for r in range(10) if r not in rows]
        for layout in LAYOUTS:
            pd, pa = _layout(p, layout, dev)
            for scaler in (None, SCALER):
                table = torch.full((10, H, 8), SENTINEL, device=dev, dtype=torch.float64)
                window_stats(torch.from_numpy(first[0]).to(dev), torch.from_numpy(first[1]).to(dev), table, rows_d, 0, scaler)
                window_stats(pd, td if layout != "model" else _layout(t, "model", dev)[0], table, rows_d, 0, scaler)
                want, mags = SR.window_table(pa, t, scaler)
                got = table.cpu().numpy()
                what = (I, H, S, layout, scaler)
                _assert_table(got[rows], want, mags, what)
                assert (got[others] == SENTINEL).all(), what
    # row0 without a row list: consecutive rows
    table = torch.full((10, H, 8), SENTINEL, device=dev, dtype=torch.float64)
    window_stats(pd, td, table, None, 3, None)
    got = table.cpu().numpy()
    _assert_table(got[3:3 + S], *SR.window_table(pa, t, None), (I, H, "row0"))
    assert (got[:3] == SENTINEL).all() and (got[3 + S:] == SENTINEL).all()
    check_device_errors()


def test_window_statistics_at_the_grid_size_sum_to_the_pooled_statistics_and_repeat(dev):
    """I = 2911 (41 x 71: 46 tiles, the last one ragged), H = 12, S = 5: the model's layout against a baseline-shaped truth
    and the other way round; the table summed over the windows against `HorizonMetrics.stats` at the same bar (the pooled
    kernel adds the same terms in another order); three launches give the same bits."""
    from src.evaluation.metrics import HorizonMetrics
    from tecmollm.significance import window_stats
    S, H, I = 5, 12, 2911
    rng = np.random.default_rng(2911)
    p, t = _hard(S, H, I, rng)
    for p_layout, t_layout in (("model", "contiguous"), ("baseline", "model")):
        pd, pa = _layout(p, p_layout, dev)
        td, ta = _layout(t, t_layout, dev)
        want, mags = SR.window_table(pa, ta, SCALER)
        tables = []
        for _ in range(3):
            table = torch.zeros(S, H, 8, device=dev, dtype=torch.float64)
            window_stats(pd, td, table, None, 0, SCALER)
            tables.append(table)
        assert torch.equal(tables[0], tables[1]) and torch.equal(tables[0], tables[2])
        _assert_table(tables[0].cpu().numpy(), want, mags, (p_layout, t_layout))
        hm = HorizonMetrics(H, SCALER, device=dev)
        hm.update(pd, td)
        pooled, total = hm.stats.cpu().numpy(), tables[0].sum(dim=0).cpu().numpy()
        assert np.array_equal(pooled[:, 0], total[:, 0]) and (total[:, 0] == S * I).all()
        err = np.abs(pooled - total) / mags.sum(axis=0)
        print(f"{p_layout}/{t_layout}: max |sum of windows - HorizonMetrics| / sum|terms| = {err.max():.3e}")
        assert (err <= BAR).all()


def test_a_bad_row_index_raises_and_writes_nothing(dev):
    from tecmollm import TecmError, check_device_errors
    from tecmollm.significance import WindowScores, window_stats
    S, H, I = 4, 3, 70
    rng = np.random.default_rng(5)
    p, t = _hard(S, H, I, rng)
    pd, td = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
    want, mags = SR.window_table(p, t, None)
    check_device_errors()
    for bad in (6, -1, 1 << 40):
        table = torch.full((6, H, 8), SENTINEL, device=dev, dtype=torch.float64)
        rows = torch.tensor([2, bad, 5, 0], dtype=torch.int64, device=dev)
        window_stats(pd, td, table, rows, 0, None)
        with pytest.raises(TecmError, match="TECM_BAD_ROW"):
            check_device_errors()
        check_device_errors()                                              # reported once, then clear
        got = table.cpu().numpy()
        _assert_table(got[[2, 5, 0]], want[[0, 2, 3]], mags[[0, 2, 3]], bad)
        assert (got[[1, 3, 4]] == SENTINEL).all()
    table = torch.full((6, H, 8), SENTINEL, device=dev, dtype=torch.float64)
    window_stats(pd, td, table, None, 3, None)                             # rows 3, 4, 5 and 6: the last one is outside
    with pytest.raises(TecmError, match="TECM_BAD_ROW"):
        check_device_errors()
    assert (table[:3] == SENTINEL).all() and (table[3:] != SENTINEL).all()
    ws = WindowScores(3, H, ["A"], None, dev)
    ws.update("A", pd, td, [0, 1, 2, 3])
    with pytest.raises(TecmError, match="TECM_BAD_ROW"):
        check_device_errors()
    with pytest.raises(ValueError):
        ws.update("A", pd, td, [0, 1])
    with pytest.raises(KeyError):
        ws.update("B", pd, td, [0, 1, 2, 0])


# ------------------------------------------------------------------------------------ bootstrap
def _group_ids(S, G, rng):
    """Group 1 is empty, the last group holds one window (when there are two windows), the rest is group 0."""
    ids = np.zeros(S, dtype=np.int32)
    if G > 1 and S > 1:
        ids[int(rng.integers(S))] = G - 1
    return ids


def _boot(table, starts, L, ids, G, dev, spread=False):
    from tecmollm.significance import bootstrap_sums
    d = torch.from_numpy(table).to(dev)
    if spread:                                                             # a non-contiguous m stride
        big = torch.full((2 * table.shape[0],) + table.shape[1:], 1e300, device=dev, dtype=torch.float64)
        big[::2] = d
        d = big[::2]
    return bootstrap_sums(d, torch.from_numpy(starts).to(dev), L, None if ids is None else torch.from_numpy(ids).to(dev), G)


@pytest.mark.parametrize("W", [1, 8, 63, 64, 65, 96, 400])
@pytest.mark.parametrize("S", [1, 2, 7, 64, 257])
def test_bootstrap_sums_are_the_sequential_restatement_bit_for_bit(dev, S, W):
    """Every block length in {1, 2, 3, S, S + 5} x (M, G, R) in {(1, 1, 1), (3, 3, 5), (3, 1, 130)}, the three-forecast table
    behind a non-contiguous m stride; G = 3 with one empty and one single-window group."""
    from tecmollm.devcheck import check_device_errors
    from tecmollm.significance import draw_starts
    rng = np.random.default_rng(1000 * S + W)
    full = rng.standard_normal((3, S, W)) * np.exp(rng.uniform(-20, 20, size=(3, S, W)))
    for L in sorted({1, 2, 3, S, S + 5}):
        for M, G, R in ((1, 1, 1), (3, 3, 5), (3, 1, 130)):
            table = np.ascontiguousarray(full[:M])
            ids = _group_ids(S, G, rng) if G > 1 else None
            starts = draw_starts(S, L, R, seed=S + L + R).numpy()
            want = SR.bootstrap_sums(table, starts, L, ids, G)
            got = _boot(table, starts, L, ids, G, dev, spread=M > 1)
            assert got.shape == (R, M, G, W) and got.dtype == torch.float64
            assert np.array_equal(got.cpu().numpy(), want), (S, W, L, M, G, R)
            if G > 1:
                assert (want[:, :, 1] == 0).all()
    check_device_errors()
    # L >= S with start 0: the plain totals, exactly
    zero = np.zeros((1, 1), dtype=np.int32)
    total = np.zeros((3, W))
    for s in range(S):
        total += full[:, s]
    assert np.array_equal(_boot(full, zero, S + 5, None, 1, dev).cpu().numpy()[0, :, 0], total)


def test_bootstrap_reports_bad_starts_and_bad_groups_and_repeats(dev):
    from tecmollm import TecmError, check_device_errors
    from tecmollm.significance import draw_starts
    S, W, L, R, G = 50, 70, 7, 6, 2
    rng = np.random.default_rng(9)
    table = rng.standard_normal((2, S, W))
    ids = (np.arange(S) % 2).astype(np.int32)
    starts = draw_starts(S, L, R, seed=3).numpy()
    outs = [_boot(table, starts, L, ids, G, dev) for _ in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    check_device_errors()
    for bad in (S, -1):
        st = starts.copy()
        st[4, 2] = bad
        got = _boot(table, st, L, ids, G, dev).cpu().numpy()
        with pytest.raises(TecmError, match="TECM_BAD_START"):
            check_device_errors()
        check_device_errors()
        assert np.array_equal(got, SR.bootstrap_sums(table, st, L, ids, G))          # the block is skipped
    for bad in (G, -1):
        ids2 = ids.copy()
        ids2[17] = bad
        got = _boot(table, starts, L, ids2, G, dev).cpu().numpy()
        with pytest.raises(TecmError, match="TECM_BAD_GROUP"):
            check_device_errors()
        check_device_errors()
        assert np.array_equal(got, SR.bootstrap_sums(table, starts, L, ids2, G))     # the window is skipped


def test_block_bootstrap_coverage_on_ar1_columns(dev):
    """One launch per block length over a (1, 512, 400) table whose columns are independent AR(1) series (phi = 0.6), R =
    300: the share of columns whose 90 % interval of the mean covers the true mean 0 lies in [0.78, 0.95] at L = 32 and is
    at most 0.70 at L = 1, where the resample ignores the dependence."""
    from tecmollm.significance import draw_starts
    x = SR.ar1_columns()
    S, C = x.shape
    cover = {}
    for L in (1, 32):
        starts = draw_starts(S, L, 300, seed=11).numpy()
        got = _boot(x[None], starts, L, None, 1, dev).cpu().numpy()
        cover[L] = SR.coverage_of_zero(got[:, 0, 0], S)
    print(f"coverage of 0 by the 90 % interval on the device: L = 1 {cover[1]:.3f}, L = 32 {cover[32]:.3f}")
    assert cover[1] <= 0.70
    assert 0.78 <= cover[32] <= 0.95


# ------------------------------------------------------------------------------------ end to end
CFG_KW = dict(L_in=16, L_out=12, num_nodes=12)
KEYS = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg", "mae_by_horizon", "rmse_by_horizon", "r2_by_horizon",
        "pearson_by_horizon")


@pytest.fixture(scope="module")
def split(dev, golden_dir):
    from oracle import ref_cpu as R
    from src.data.dataset import SlidingWindowSamplerDataset
    from tests.parity import build_model
    cfg = R.default_config(**CFG_KW)
    model = build_model(cfg, R.init_params(cfg, seed=3), dev, "per_timestep").eval()
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev)
    g = np.load(os.path.join(golden_dir, "evaluate_split.npz"))
    ds = SlidingWindowSamplerDataset.from_tensors(torch.as_tensor(g["X"]), torch.as_tensor(g["Y"]), torch.as_tensor(g["TF"]),
                                                  int(g["L_in"]), int(g["L_out"]), stride=1, device=dev, mode="test")
    return model, ds, ei, (float(g["mean"]), float(g["scale"]))


def _numbers(obj, path=""):
    """Every number and array of a nested result, flattened to {path: float64 array}; the `WindowScores` as its table."""
    if isinstance(obj, dict):
        out = {}
        for k, v in obj.items():
            out.update(_numbers(v, f"{path}/{k}"))
        return out
    if isinstance(obj, (list, tuple)) and not all(isinstance(v, str) for v in obj):
        out = {}
        for n, v in enumerate(obj):
            out.update(_numbers(v, f"{path}/{n}"))
        return out
    if hasattr(obj, "table"):
        return {path: obj.table.cpu().numpy()}
    if isinstance(obj, (str, list, tuple)):
        return {}
    return {path: np.asarray(obj, dtype=np.float64)}


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_significance_end_to_end_on_a_tiny_model(dev, split, tmp_path):
    """12 nodes, 24 windows, batch size 5 (a ragged last batch), two baselines, three groups of windows."""
    from tecmollm import conformal as CF
    from tecmollm import evaluate as E
    from tecmollm import significance as SG
    model, ds, ei, scaler = split
    S, H = len(ds), 12
    base = ("mean", "last")
    slots = (torch.arange(S, device=dev) % 3).to(torch.int32)
    want = E.evaluate_split(model, ds, ei, 5, scaler=scaler, baselines=base)
    res, sig = SG.evaluate_significance(model, ds, ei, 5, scaler=scaler, baselines=base, replicates=60, seed=1, groups=slots,
                                        num_groups=3)
    assert res == want and list(res) == list(want)
    scores = sig["scores"]
    assert scores.names == ["TEC-MoLLM", "HistoricalAverage", "Persistence"] and scores.table.shape == (3, S, H, 8)
    assert (scores.L_in, scores.L_out, scores.stride) == (16, 12, 1) and sig["block_len"] == SG.default_block_len(S, 16, 12, 1) == 3
    assert (scores.table[..., 0] == 12).all()                              # every window written: 12 nodes each
    # the table is the restatement of every batch's forecasts, and its sum the pooled statistics
    with torch.no_grad():
        x, tf, y = ds.batch(list(range(5)))
        out = model(x, tf, ei)
    ref, mags = SR.window_table(out.squeeze(-1).cpu().numpy(), y.squeeze(-1).cpu().numpy(), scaler)
    _assert_table(scores.table[0, :5].cpu().numpy(), ref, mags, "first batch")
    totals = scores.totals()
    assert totals.shape == (3, H, 8) and np.array_equal(totals, scores.table.cpu().numpy().cumsum(axis=1)[:, -1])
    # the hook changes nothing: evaluate_maps and evaluate_conformal return the same bits, and a pass with the hook too
    res_m, maps = E.evaluate_maps(model, ds, ei, 5, scaler=scaler, baselines=base, groups=slots, num_groups=3)
    seen = []
    with torch.no_grad():
        hms, mms = E._score_pass(model, ds, ei, 5, scaler, base, None, None, slots, 3,
                                 per_forecast=lambda name, pred, y, chunk: seen.append((name, list(chunk))))
    assert [s[0] for s in seen[:3]] == scores.names and seen[0][1] == [0, 1, 2, 3, 4] and len(seen) == 3 * 5
    iv = CF.calibrate_conformal(model, ds, ei, 5, alpha=0.2, scaler=scaler, order=list(range(14)))
    res_c, maps_c, _ = CF.evaluate_conformal(model, ds, ei, 5, iv, groups=slots, num_groups=3, baselines=base)
    for name in want:
        hooked = mms[name].compute()
        for k in KEYS:
            assert res_m[name][k] == want[name][k] == res_c[name][k] == hms[name].compute()[k], (name, k)
        for k in maps[name]:
            if k != "by_group":
                assert np.array_equal(maps[name][k], hooked[k], equal_nan=True), (name, k)
                assert np.array_equal(maps[name][k], maps_c[name][k], equal_nan=True), (name, k)
    # the same seed gives the same sig, another seed another resample
    again = SG.evaluate_significance(model, ds, ei, 5, scaler=scaler, baselines=base, replicates=60, seed=1, groups=slots,
                                     num_groups=3)[1]
    other = SG.evaluate_significance(model, ds, ei, 5, scaler=scaler, baselines=base, replicates=60, seed=2, groups=slots,
                                     num_groups=3)[1]
    assert _same(_numbers(sig), _numbers(again)) and not _same(_numbers(sig), _numbers(other))
    assert torch.equal(other["scores"].table, scores.table)
    # lo <= hi everywhere, p_better a share, the shapes
    for name, ivs in sig["intervals"].items():
        assert ivs["baseline"] == name and ivs["model"] == "TEC-MoLLM" and ivs["num_groups"] == 3
        bands = [b for per in ivs["metrics"].values() for b in per.values()] + list(ivs["improvement"].values())
        for band in bands:
            ok = ~np.isnan(band["lo"])
            assert (band["lo"][ok] <= band["hi"][ok]).all() and ok.any() and (band["nan_replicates"] <= 60).all()
        assert ivs["metrics"][name]["mae"]["point"].shape == (3, H) and ivs["improvement"]["rmse"]["lo"].shape == (3,)
        for k in ("mae", "rmse"):
            assert ((0 <= ivs["p_better"][k]) & (ivs["p_better"][k] <= 1)).all()
        for loss in ("se", "ae"):
            dm = sig["dm"][name][loss]
            assert len(dm) == 3 and [g["n"] for g in dm] == [8, 8, 8] and dm[0]["stat"].shape == (H,)
            assert all(math.isnan(g["p_pooled"]) or 0 <= g["p_pooled"] <= 1 for g in dm)
    # one group: the point values are evaluate_split's numbers and improvement()'s percentages
    boot = SG.block_bootstrap(scores, 40, None, 7)
    assert boot.shape == (40, 3, 1, H, 8) and boot.is_cuda and boot.dtype == torch.float64
    assert (boot[..., 0].sum(dim=(2, 3)) == S * H * 12).all()              # every replicate reads exactly S windows
    one = SG.bootstrap_intervals(boot, scores, 0.9)
    imp = E.improvement(want)
    for k in SG.IMPROVEMENTS:
        np.testing.assert_allclose(one["improvement"][k]["point"][0], imp[k], rtol=1e-9)
    for name in want:
        for k in SG.AVERAGES:
            np.testing.assert_allclose(one["metrics"][name][k]["point"][0], want[name][k], rtol=1e-10)
    # the model against itself: the improvement is exactly 0 in every replicate, and the test has nothing to test
    own = SG.bootstrap_intervals(boot, scores, 0.9, "TEC-MoLLM", "TEC-MoLLM")
    for k in ("mae", "rmse"):
        band = own["improvement"][k]
        assert band["lo"][0] == 0.0 and band["hi"][0] == 0.0 and band["point"][0] == 0.0
        assert own["p_better"][k][0] == 0.0
    dm = SG.diebold_mariano(scores, "TEC-MoLLM", "TEC-MoLLM")
    assert np.isnan(dm["stat"]).all() and math.isnan(dm["stat_pooled"]) and math.isnan(dm["p_pooled"]) and dm["n"] == S
    real = SG.diebold_mariano(scores, "TEC-MoLLM", "HistoricalAverage", "ae")
    assert np.isfinite(real["stat"]).all() and real["lags"] == SG.default_lags(S, 12, 1) == 11
    d = (scores.table[0, :, :, 6] / scores.table[0, :, :, 0] - scores.table[1, :, :, 6] / scores.table[1, :, :, 0]).cpu().numpy()
    stat, p = SR.dm(d.mean(axis=1), 11)
    np.testing.assert_allclose([real["stat_pooled"], real["p_pooled"]], [stat, p], rtol=1e-9)
    # two halves of the split written into one table by hand are the full pass's table (batches of 4: the same batches)
    full = SG.score_windows(model, ds, ei, 4, scaler, base)[1]
    hand = SG.WindowScores(S, H, full.names, scaler, dev)
    for half in (list(range(12, 24)), list(range(12))):
        with torch.no_grad():
            E._score_pass(model, ds, ei, 4, scaler, base, None, half, None, None,
                          per_forecast=lambda name, pred, y, chunk: hand.update(name, pred, y, chunk))
    assert torch.equal(hand.table, full.table)
    first = SG.score_windows(model, ds, ei, 4, scaler, base, order=list(range(12)))[1]
    assert torch.equal(first.table[:, :12], full.table[:, :12]) and float(first.table[:, 12:].abs().sum()) == 0.0
    # the files
    paths = SG.write_significance(sig, str(tmp_path / "out"))
    assert sorted(os.listdir(tmp_path / "out")) == ["significance.csv", "significance.npz"]
    with open(paths["csv"], encoding="utf-8") as f:
        lines = f.read().splitlines()
    assert lines[0] == ",".join(SG.CSV_COLUMNS) and len(lines) == 1 + (2 + 2) * 3 * 4   # model x 2 baselines + 2 baselines
    z = np.load(paths["npz"])
    assert z["TEC-MoLLM/mae_avg"].shape == (60, 3) and z["improvement/Persistence/rmse"].shape == (60, 3)
    assert len(z.files) == 3 * 4 + 2 * 4
    back = SG.WindowScores.load(scores.save(str(tmp_path / "scores.npz")), dev)
    assert torch.equal(back.table, scores.table) and back.names == scores.names and back.scaler == scores.scaler
    assert (back.L_in, back.L_out, back.stride) == (16, 12, 1)
