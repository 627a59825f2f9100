"""GPU tests of the per-cell evaluation statistics: the kernel (tecm_metrics_map) through `MapMetrics` against a float64
numpy restatement that adds in the kernel's order (tests/error_maps_ref.py), against `HorizonMetrics`, against the
reference's own per-cell metrics (tools/make_golden_error_maps.py), its determinism, its group-id check, the grouping
helpers on a device-resident dataset and `evaluate_maps` end to end on a tiny model.

The bar of every comparison with the restatement: per statistic |kernel - numpy| <= 1e-12 * sum |terms|, the sum taken from
the restatement.  Same order of additions on both sides, so only FMA contraction and at most ~50 float64 roundings lie
between them, about 6e-15 of sum |terms|: two orders of margin, derived and not measured."""
import os

import numpy as np
import pytest
import torch

from tests.error_maps_ref import accumulate, pipeline

pytestmark = pytest.mark.gpu

KEYS = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg", "mae_by_horizon", "rmse_by_horizon", "r2_by_horizon",
        "pearson_by_horizon")
MAP_KEYS = ("count", "mae", "rmse", "bias", "r2_score", "pearson_r")
BAR = 1e-12
SCALER = (21.5, 9.25)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _inject(a, rng):
    """NaN, +inf, -inf at three distinct places of a float32 array with at least six elements (else none)."""
    flat = a.reshape(-1)
    if flat.size >= 6:
        where = rng.choice(flat.size, size=3, replace=False)
        flat[where[0]], flat[where[1]], flat[where[2]] = np.nan, np.inf, -np.inf
    return a


def _operands(layout, S, H, I, rng, dev):
    """(pred view on the device, true view on the device, pred (S, H, I') numpy, true numpy, I').  The views have the
    strides the layout is named after; the numpy arrays are what they hold, as (S, H, I')."""
    def values(*shape):
        return _inject((rng.standard_normal(shape) * 2.5).astype(np.float32), rng)
    if layout == "model":                          # the model's output: (B, N, L_out) permuted, stride_h = 1, stride_i = H
        p = values(S, I, H)
        pd, pn = torch.from_numpy(p).to(dev).permute(0, 2, 1).unsqueeze(-1), p.transpose(0, 2, 1)
        t = values(S, H, I)
        td, tn = torch.from_numpy(t).to(dev).unsqueeze(-1), t
    elif layout == "contiguous":                   # node-fastest forecast; the target takes the permuted layout here
        p = values(S, H, I)
        pd, pn = torch.from_numpy(p).to(dev), p
        t = values(S, I, H)
        td, tn = torch.from_numpy(t).to(dev).permute(0, 2, 1), t.transpose(0, 2, 1)
    elif layout == "baseline":                     # one value per (window, node) as a view with stride_h = 0
        p = values(S, I)
        pd = torch.from_numpy(p).to(dev).view(S, 1, I, 1).expand(S, H, I, 1)
        pn = np.broadcast_to(p[:, None, :], (S, H, I))
        t = values(S, H, I)
        td, tn = torch.from_numpy(t).to(dev).unsqueeze(-1), t
    elif layout == "strided":                      # every second node of a wider tensor: stride_i = 2
        p = values(S, H, 2 * I)
        pd, pn = torch.from_numpy(p).to(dev)[:, :, ::2], p[:, :, ::2]
        t = values(S, H, 2 * I + 1)
        td, tn = torch.from_numpy(t).to(dev)[:, :, 1::2], t[:, :, 1::2]
    elif layout == "fallback":                     # trailing dims (2, I) cut out of (2, I + 1): no single stride
        p = values(S, H, 2, I + 1)
        pd, pn = torch.from_numpy(p).to(dev)[..., :I], p[..., :I].reshape(S, H, 2 * I)
        t = values(S, H, 2, I)
        td, tn = torch.from_numpy(t).to(dev), t.reshape(S, H, 2 * I)
        I = 2 * I
    else:
        raise AssertionError(layout)
    return pd, td, np.ascontiguousarray(pn), np.ascontiguousarray(tn), I


def _assert_close(got, want, mags, what):
    err = np.abs(got - want)
    bound = BAR * mags
    worst = float(np.max(err / np.maximum(mags, 1e-300)))
    print(f"{what}: max |kernel - numpy| / sum|terms| = {worst:.3e}")
    assert np.all(err <= bound), (what, worst)


@pytest.mark.parametrize("layout", ["model", "contiguous", "baseline", "strided", "fallback"])
def test_statistics_match_the_ordered_float64_restatement(dev, layout):
    """I over tile edges (1, 63, 64, 65, 135), H = 1, 12, 24 and 50 (above TECM_MAP_LDS_MAX_H = 32), S = 1 and 5, G = 1
    and 3 (ids out of order, group 1 never visited and pre-filled with a sentinel), with and without scaler + clip, NaN and
    both infinities in both operands, two consecutive updates into the same object."""
    from src.evaluation.metrics import MapMetrics, _as_shi
    from tecmollm import _lib
    assert _lib.TECM_MAP_LDS_MAX_H == 32
    rng = np.random.default_rng(sum(map(ord, layout)))
    for I0 in (1, 63, 64, 65, 135):
        for H in (1, 12, 24, 50):
            for S in (1, 5):
                for G in (1, 3):
                    scaler = SCALER if (I0 + H + S + G) % 2 else None
                    mm, want, mags = None, None, None
                    for update in range(2):
                        pd, td, pn, tn, I = _operands(layout, S, H, I0, rng, dev)
                        if layout == "fallback" and I0 > 1:
                            assert _as_shi(pd, "p")[0].data_ptr() != pd.data_ptr()           # a copy was needed
                        elif layout != "fallback":
                            assert _as_shi(pd, "p")[0].data_ptr() == pd.data_ptr()           # read in place
                        if mm is None:
                            mm = MapMetrics(H, I, G, scaler, device=dev)
                            want, mags = np.zeros((G, H, 8, I)), np.zeros((G, H, 8, I))
                            if G == 3:
                                sentinel = torch.arange(H * 8 * I, device=dev, dtype=torch.float64).view(H, 8, I) + 0.5
                                mm.stats[1].copy_(sentinel)
                        ids = None
                        if G == 3:
                            ids = np.array([2, 0, 2, 0, 2][:S] if update == 0 else [0, 2, 2, 0, 0][:S], dtype=np.int32)
                        elif update == 1:
                            ids = np.zeros(S, dtype=np.int32)                                  # the same as None
                        mm.update(pd, td, None if ids is None else torch.from_numpy(ids).to(dev))
                        accumulate(want, mags, pn, tn, ids, scaler)
                    got = mm.stats.cpu().numpy()
                    what = f"{layout} I={I} H={H} S={S} G={G} scaler={scaler is not None}"
                    if G == 3:
                        assert torch.equal(mm.stats[1], sentinel), what + ": the never-visited group was touched"
                        got[1] = want[1] = 0
                    _assert_close(got, want, mags, what)
                    assert np.array_equal(got[:, :, 0], want[:, :, 0])                         # the counts, exactly
    from tecmollm import check_device_errors
    check_device_errors()                                                                      # no id was out of range


def _full_batches(dev, batches=3, B=16, N=2911, H=12, seed=0):
    """Model-style predictions (permuted (B, N, H)) and dataset-style targets ((B, H, N, 1)), with a few non-finite values."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(batches):
        p = _inject((rng.standard_normal((B, N, H)) * 1.5).astype(np.float32), rng)
        t = _inject((rng.standard_normal((B, H, N)) * 1.5).astype(np.float32), rng)
        out.append((torch.from_numpy(p).to(dev).permute(0, 2, 1).unsqueeze(-1), torch.from_numpy(t).to(dev).unsqueeze(-1),
                    p.transpose(0, 2, 1), t))
    return out


def test_collapse_agrees_with_horizon_metrics_and_three_runs_are_bit_identical(dev):
    """N = 2911, H = 12, B = 16, three batches, four groups.  collapse() against HorizonMetrics.stats fed the same batches:
    the order of additions differs there (and HorizonMetrics adds with atomics), so the bar is on sum |terms| too.  Three
    fresh accumulations hold the same bits: one owner per cell, no atomics."""
    from src.evaluation.metrics import HorizonMetrics, MapMetrics
    batches = _full_batches(dev)
    ids = [torch.from_numpy(((np.arange(16) * 7 + b) % 4).astype(np.int32)).to(dev) for b in range(3)]
    runs = []
    for _ in range(3):
        mm = MapMetrics(12, 2911, 4, SCALER, device=dev)
        for (pd, td, _, _), g in zip(batches, ids):
            mm.update(pd, td, g)
        runs.append(mm.stats.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    hm = HorizonMetrics(12, SCALER, device=dev)
    for pd, td, _, _ in batches:
        hm.update(pd, td)
    want, mags = np.zeros((1, 12, 8, 2911)), np.zeros((1, 12, 8, 2911))
    for _, _, pn, tn in batches:
        accumulate(want, mags, pn, tn, None, SCALER)
    mags = mags.sum(axis=(0, 3))
    _assert_close(mm.collapse(), hm.stats.cpu().numpy(), mags, "collapse vs HorizonMetrics")
    _assert_close(mm.collapse(), want.sum(axis=(0, 3)), mags, "collapse vs numpy")
    assert mm.collapse()[:, 0].tolist() == [48.0 * 2911] * 12


def test_map_metrics_match_the_reference_cell_by_cell(dev, golden_dir):
    """The inputs of tests/golden/error_maps.npz through the kernel, in both operand layouts: the reference's per-cell
    MAE / RMSE / R^2 / Pearson r at rtol 2e-5 (the reference sums in float32)."""
    from src.evaluation.metrics import MapMetrics
    g = np.load(os.path.join(golden_dir, "error_maps.npz"))
    scaler = (float(g["mean"]), float(g["scale"]))
    p, t = torch.from_numpy(g["y_pred"]).to(dev), torch.from_numpy(g["y_true"]).to(dev)
    for pred in (p, p.permute(0, 2, 1).contiguous().permute(0, 2, 1)):
        mm = MapMetrics(3, 5, 1, scaler, device=dev)
        mm.update(pred[:25], t[:25])
        mm.update(pred[25:], t[25:])
        out = mm.compute()
        assert set(out) == set(MAP_KEYS) | {"by_group"} and set(out["by_group"][0]) == set(KEYS)
        assert (out["count"] == 40).all()
        for k in ("mae", "rmse", "r2_score", "pearson_r"):
            assert out[k].shape == (1, 3, 5)
            np.testing.assert_allclose(out[k][0], g[f"out_{k}"], rtol=2e-5, atol=0, err_msg=k)
        tt, pp = pipeline(g["y_pred"], g["y_true"], scaler)
        np.testing.assert_allclose(out["bias"][0], (pp.astype(np.float64) - tt).mean(axis=0), rtol=1e-11, atol=1e-12)


def test_a_group_id_out_of_range_is_skipped_and_reported(dev):
    """One sample with id = G (and, in a second object, one with id -1): the other samples are accumulated, no cell takes
    the bad sample, and check_device_errors() raises TecmError naming TECM_BAD_GROUP.  An error flag, not a fault."""
    from src.evaluation.metrics import MapMetrics
    from tecmollm import TecmError, check_device_errors
    check_device_errors()
    rng = np.random.default_rng(12)
    for bad in (3, -1):
        S, H, I, G = 5, 12, 65, 3
        pd, td, pn, tn, _ = _operands("model", S, H, I, rng, dev)
        ids = np.array([0, bad, 1, 2, 0], dtype=np.int32)
        mm = MapMetrics(H, I, G, SCALER, device=dev)
        mm.update(pd, td, torch.from_numpy(ids).to(dev))
        want, mags = np.zeros((G, H, 8, I)), np.zeros((G, H, 8, I))
        accumulate(want, mags, pn, tn, ids, SCALER)                        # skips the sample, as the kernel must
        got = mm.stats.cpu().numpy()
        _assert_close(got, want, mags, f"bad id {bad}")
        assert got[:, :, 0].sum() == 4 * H * I                             # four samples counted, nowhere a fifth
        with pytest.raises(TecmError, match="TECM_BAD_GROUP"):
            check_device_errors()
        check_device_errors()                                              # reported once, then clear


def _time_features(T):
    t = torch.arange(T, dtype=torch.float32)
    return torch.stack([(t * 5) % 12, t % 366, torch.zeros(T), (t // 30) % 4], 1)


def _dataset(X, L_in, L_out, stride, dev, Y=None, TF=None):
    from src.data.dataset import SlidingWindowSamplerDataset
    X = torch.as_tensor(X)
    T, H, W, _ = X.shape
    Y = torch.zeros(T, H, W, L_out) if Y is None else torch.as_tensor(Y)
    TF = _time_features(T) if TF is None else torch.as_tensor(TF)
    return SlidingWindowSamplerDataset.from_tensors(X, Y, TF, L_in, L_out, stride=stride, device=dev, mode="test")


def test_window_groups_on_a_resident_dataset_match_a_host_loop(dev):
    """A 60-step split at dataset stride 3 whose channel 4 is a Kp-like series of whole numbers, feature-scaled: both spans,
    the three reductions, edges that hit values exactly; and the time-of-day slot of every window's first target step."""
    from tecmollm.evaluate import window_groups_by_index, window_groups_by_slot
    T, L_in, L_out, stride = 60, 7, 4, 3
    kp = np.round(4 + 3.9 * np.sin(np.arange(T) / 5.0)).astype(np.float32)
    mean, scale = 3.5, 2.0
    X = np.random.default_rng(1).standard_normal((T, 3, 4, 6)).astype(np.float32)
    X[..., 4] = ((kp - mean) / scale)[:, None, None]                       # one value per step, broadcast over the grid
    ds = _dataset(X, L_in, L_out, stride, dev)
    starts = list(range(0, T - L_in - L_out + 1, stride))
    assert ds.sample_indices == starts
    edges = [2.0, 4.0, 6.0]

    class FeatureScaler:                                                   # what a fitted StandardScaler over X's channels exposes
        mean_ = np.array([0, 0, 0, 0, mean, 0.0])
        scale_ = np.array([1, 1, 1, 1, scale, 1.0])
    for span in ("input", "target"):
        for reduce in ("max", "min", "last"):
            want = []
            for a in starts:
                win = kp[a:a + L_in] if span == "input" else kp[a + L_in:a + L_in + L_out]
                v = {"max": win.max(), "min": win.min(), "last": win[-1]}[reduce]
                want.append(sum(1 for e in edges if e < v))
            for fs in (FeatureScaler, (mean, scale)):
                got = window_groups_by_index(ds, 4, edges, span=span, feature_scaler=fs, reduce=reduce)
                assert got.is_cuda and got.dtype == torch.int32 and got.shape == (len(ds),)
                assert got.tolist() == want, (span, reduce)
            assert len(set(want)) > 1
    assert window_groups_by_index(ds, 4, edges).tolist() == window_groups_by_index(ds, 4, edges, "target", None, "max").tolist()
    slots = window_groups_by_slot(ds)
    tf = _time_features(T)
    assert slots.is_cuda and slots.dtype == torch.int32
    assert slots.tolist() == [int(tf[a + L_in, 0]) for a in starts]
    with pytest.raises(ValueError):
        window_groups_by_index(ds, 6, edges)


# ------------------------------------------------------------------------------------ evaluate_maps end to end
@pytest.fixture(scope="module")
def split(dev, golden_dir):
    from oracle import ref_cpu as R
    from tests.parity import build_model
    g = np.load(os.path.join(golden_dir, "evaluate_split.npz"))
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=12)
    model = build_model(cfg, R.init_params(cfg, seed=3), dev, "per_timestep").eval()
    ds = _dataset(g["X"], int(g["L_in"]), int(g["L_out"]), 1, dev, Y=g["Y"], TF=g["TF"])
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev)
    return g, model, ds, ei, (float(g["mean"]), float(g["scale"]))


def test_evaluate_maps_end_to_end_on_a_tiny_model(dev, split):
    """12 nodes, 24 windows, batch size 5 (a ragged last batch).  The first result is evaluate_split's, key by key and
    exactly; the maps of a forecast pool to its HorizonMetrics numbers; with the windows grouped by time-of-day slot every
    window lands in the group a host loop assigns; two shards added by hand give the full split's maps."""
    from src.evaluation.metrics import MapMetrics
    from tecmollm import evaluate as E
    g, model, ds, ei, scaler = split
    S, N, H = len(ds), 12, 12
    assert S % 5 != 0
    want = E.evaluate_split(model, ds, ei, 5, scaler=scaler, baselines=("mean", "last"))
    res, maps = E.evaluate_maps(model, ds, ei, 5, scaler=scaler, baselines=("mean", "last"))
    assert list(res) == list(want) == list(maps) == ["TEC-MoLLM", "HistoricalAverage", "Persistence"]
    for name in want:
        assert set(res[name]) == set(want[name]) == set(KEYS)
        for k in KEYS:
            assert res[name][k] == want[name][k], (name, k)                # exactly
        assert maps[name]["count"].shape == (1, H, N) and (maps[name]["count"] == S).all()
        pooled = maps[name]["by_group"][0]                                 # one group: the pooled dict is the forecast's own
        for k in KEYS:
            np.testing.assert_allclose(np.asarray(pooled[k]), np.asarray(want[name][k]), rtol=1e-12, atol=0, err_msg=name + k)
    # grouped by the slot of the first target step
    slots = E.window_groups_by_slot(ds)
    host = [int(g["TF"][a + ds.L_in, 0]) for a in ds.sample_indices]
    assert slots.tolist() == host
    res12, maps12 = E.evaluate_maps(model, ds, ei, 5, scaler=scaler, groups=slots, num_groups=12)
    for k in KEYS:
        assert res12["TEC-MoLLM"][k] == want["TEC-MoLLM"][k]
    for name in ("TEC-MoLLM", "HistoricalAverage"):
        count = maps12[name]["count"]
        assert count.shape == (12, H, N) and count.sum() == S * N * H
        for s in range(12):
            assert (count[s] == host.count(s)).all(), (name, s)
        empty = [s for s in range(12) if host.count(s) == 0]
        for s in empty:                                                    # a slot the split never visits reads NaN
            assert np.isnan(maps12[name]["mae"][s]).all() and np.isnan(maps12[name]["by_group"][s]["mae_avg"])
    # two shards (what two ranks' sampler halves would be), statistics added by hand
    halves = [list(range(0, S, 2)), list(range(1, S, 2))]
    kept = []
    orig = MapMetrics.compute

    def spy(self):
        kept.append(self.stats.clone())
        return orig(self)
    MapMetrics.compute = spy
    try:
        for h in halves:
            E.evaluate_maps(model, ds, ei, 5, scaler=scaler, groups=slots, num_groups=12, order=h)
    finally:
        MapMetrics.compute = orig
    assert len(kept) == 4
    for i, name in enumerate(["TEC-MoLLM", "HistoricalAverage"]):
        mm = MapMetrics(H, N, 12, scaler, device=dev)
        mm.stats.copy_(kept[i] + kept[2 + i])
        merged = mm.compute()
        for k in MAP_KEYS:
            np.testing.assert_allclose(merged[k], maps12[name][k], rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=name + k)
    with pytest.raises(ValueError):
        E.evaluate_maps(model, ds, ei, 5, scaler=scaler, groups=slots[:-1], num_groups=12)
    with pytest.raises(ValueError):
        E.evaluate_maps(model, ds, ei, 5, scaler=scaler, groups=slots.long(), num_groups=12)
