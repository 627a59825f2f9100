"""GPU tests of the evaluation of a test split: the per-window baseline kernel (tecm_window_baseline) and the slot-mean
kernel (tecm_slot_mean) through the C ABI, `tecmollm.evaluate` and `src.models.baselines` against golden vectors made by
the reference's own test.py / baselines.py / metrics.py (tools/make_golden_evaluate.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg", "mae_by_horizon", "rmse_by_horizon", "r2_by_horizon",
        "pearson_by_horizon")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _time_features(T):
    t = torch.arange(T, dtype=torch.float32)
    return torch.stack([t % 12, t % 366, torch.zeros(T), (t // 30) % 4], 1)


def _dataset(X, L_in, L_out, stride, dev, Y=None, TF=None):
    from src.data.dataset import SlidingWindowSamplerDataset
    X = torch.as_tensor(X)
    T, H, W, _ = X.shape
    Y = torch.zeros(T, H, W, L_out) if Y is None else torch.as_tensor(Y)
    TF = _time_features(T) if TF is None else torch.as_tensor(TF)
    return SlidingWindowSamplerDataset.from_tensors(X, Y, TF, L_in, L_out, stride=stride, device=dev, mode="test")


def _sequential_mean(x):
    """(L, ...) fp32 -> mean over axis 0: fp32 adds in ascending order, one fp32 division (the kernel's specification)."""
    acc = x[0].copy()
    for t in range(1, x.shape[0]):
        acc = acc + x[t]
    assert acc.dtype == np.float32
    return acc / np.float32(x.shape[0])


def _check(out, want, rtol, atol):
    for k in KEYS:
        np.testing.assert_allclose(np.asarray(out[k]), np.asarray(want[k]), rtol=rtol, atol=atol, err_msg=k)


def _full_split(T, seed):
    """(T, 41, 71, 6) fp32: the reference's grid (2911 nodes) with a spread of magnitudes and signs."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, 41, 71, 6), dtype=np.float32)
    return X * np.exp(rng.standard_normal((T, 41, 71, 1), dtype=np.float32))


# ------------------------------------------------------------------------------------ MEAN: the reference's bits
def test_mean_baseline_is_bit_equal_to_the_reference_function(dev, golden_dir):
    """test.py:46-71 on synthetic splits (grid 3 x 5, C = 6, L_in 7 / 16 / 48, L_out 4 / 12, dataset stride 1 / 3): the
    reference's own output, through window_baseline and through get_baseline_predictions.  No tolerance."""
    from tecmollm.evaluate import get_baseline_predictions, window_baseline
    g = np.load(os.path.join(golden_dir, "evaluate_window_mean.npz"))
    assert len(g["cases"]) == 12
    for k, (L_in, L_out, stride) in enumerate(g["cases"].tolist()):
        want = g[f"pred_{k}"]                                             # (S, H, W, L_out)
        ds = _dataset(g["X"][:L_in + L_out - 1 + 24], L_in, L_out, stride, dev)
        S, H, W, _ = want.shape
        assert len(ds) == S
        got = get_baseline_predictions(ds, L_in, L_out)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got, want), (L_in, L_out, stride)
        wb = window_baseline(ds, range(S), "mean")
        assert wb.is_cuda and wb.shape == (S, L_out, H * W, 1) and wb.stride(1) == 0
        assert np.array_equal(wb.cpu().numpy()[..., 0], want.reshape(S, H * W, L_out).transpose(0, 2, 1)), (L_in, L_out, stride)
        pick = [S - 1, 0, S // 2]                                         # any order, any subset
        wb = window_baseline(ds, pick, "mean")
        assert np.array_equal(wb.cpu().numpy()[:, 0, :, 0], want.reshape(S, H * W, L_out)[pick, :, 0])


@pytest.mark.parametrize("L_in", [48, 336])
def test_mean_baseline_full_grid_is_the_sequential_fp32_sum(dev, L_in):
    """N = 2911, C = 6, B = 8: bit-equal to a sequential fp32 numpy loop; three launches return identical bits."""
    from tecmollm.evaluate import window_baseline
    X = _full_split(L_in + 12 + 40, seed=L_in)
    ds = _dataset(X, L_in, 12, 1, dev)
    pick = [0, 3, 7, 11, 19, 23, 31, len(ds) - 1]
    want = np.stack([_sequential_mean(X[a:a + L_in, :, :, 0]).reshape(-1) for a in pick])
    runs = [window_baseline(ds, pick, "mean").cpu().numpy() for _ in range(3)]
    assert runs[0].shape == (8, 12, 2911, 1)
    assert np.array_equal(runs[0][:, 0, :, 0], want)
    assert np.array_equal(runs[0][:, 11, :, 0], want)
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    # another channel, and an output with a real horizon stride (the layout get_baseline_predictions fills)
    want3 = np.stack([_sequential_mean(X[a:a + L_in, :, :, 3]).reshape(-1) for a in pick])
    assert np.array_equal(window_baseline(ds, pick, "mean", channel=3).cpu().numpy()[:, 0, :, 0], want3)


# ------------------------------------------------------------------------------------ LAST / PERIODIC, argument checks
def test_last_and_periodic_baselines_are_plain_indexing(dev):
    from tecmollm.evaluate import window_baseline
    L_in, L_out = 48, 12
    X = _full_split(L_in + L_out + 30, seed=5)
    ds = _dataset(X, L_in, L_out, 3, dev)
    pick = list(range(len(ds)))[::2][:8]
    starts = [3 * i for i in pick]
    last = window_baseline(ds, pick, "last")
    assert last.shape == (len(pick), L_out, 2911, 1) and last.stride(1) == 0
    assert np.array_equal(last.cpu().numpy()[:, 5, :, 0], np.stack([X[a + L_in - 1, :, :, 0].reshape(-1) for a in starts]))
    for period, L_o in ((12, 12), (5, 12), (48, 12)):                     # period < L_out wraps: h mod period
        per = window_baseline(ds, pick, "periodic", period=period)
        want = np.stack([np.stack([X[a + L_in - period + h % period, :, :, 0].reshape(-1) for h in range(L_o)])
                         for a in starts])
        assert per.shape == (len(pick), L_o, 2911, 1)
        assert np.array_equal(per.cpu().numpy()[..., 0], want), period
    per2 = window_baseline(ds, pick, "periodic", channel=2, period=12)
    assert np.array_equal(per2.cpu().numpy()[0, :, :, 0], X[starts[0] + L_in - 12:starts[0] + L_in, :, :, 2].reshape(12, -1))
    runs = [window_baseline(ds, pick, kind).cpu().numpy() for kind in ("last", "periodic") for _ in range(3)]
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    assert np.array_equal(runs[3], runs[4]) and np.array_equal(runs[3], runs[5])


def test_baseline_argument_checks(dev):
    import ctypes as C
    from tecmollm import TecmError
    from tecmollm._lib import TECM_BASELINE_MEAN, TecmWindowBaseline, lib, stream_ptr
    from tecmollm.evaluate import window_baseline
    X = np.random.default_rng(0).standard_normal((40, 3, 5, 6)).astype(np.float32)
    ds = _dataset(X, 7, 4, 1, dev)
    with pytest.raises(ValueError):
        window_baseline(ds, [0, 1], "periodic", period=12)               # L_in = 7 < period
    with pytest.raises(ValueError):
        window_baseline(ds, [0], "median")
    with pytest.raises(TecmError):
        window_baseline(ds, [0, 1], "mean", channel=6)
    with pytest.raises(IndexError):
        window_baseline(ds, [len(ds)], "mean")

    def raw(start):                                                        # the entry point's own range check
        host = torch.tensor([0, start], dtype=torch.int64)
        starts = host.to(dev)
        out = torch.zeros(2, 15, device=dev)
        w = TecmWindowBaseline(X=ds.X.data_ptr(), starts=starts.data_ptr(), starts_host_check=host.data_ptr(), T=40, N=15,
                               C=6, channel=0, L_in=7, L_out=4, B=2, mode=TECM_BASELINE_MEAN, period=0,
                               out=out.data_ptr(), o_stride_b=15, o_stride_h=0, o_stride_n=1)
        rc = lib().tecm_window_baseline(C.byref(w), stream_ptr())
        torch.cuda.synchronize()
        return rc
    assert raw(33) == 0                                                    # T - L_in: the last valid start
    assert raw(34) < 0 and b"outside [0, T - L_in]" in lib().tecm_last_error()
    assert raw(-1) < 0
    from tecmollm._lib import check
    with pytest.raises(TecmError):
        check(raw(34), "tecm_window_baseline")


# ------------------------------------------------------------------------------------ slot means / HistoricalAverage
def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _f64_slot_means(tec, slots, n_slots=12):
    return np.stack([tec[slots == s].astype(np.float64).mean(axis=0) for s in range(n_slots)], axis=1)


def test_historical_average_fit_and_predict_meet_both_bars(dev, golden_dir):
    """Bar 1: float64 numpy on the same fp32 data, relative error <= 1e-12 (the kernel sums in fp64).  Bar 2: the reference's
    fit / predict (an fp32 pairwise sum: blocks of <= 128 elements on 8 accumulators, then a tree; error bound about
    (16 + 3 + ceil(log2(n / 128))) * 2^-24 ~ 1.4e-6 relative on positive data), relative error <= 2e-6."""
    from src.models.baselines import HistoricalAverage, time_slots
    g = np.load(os.path.join(golden_dir, "evaluate_historical_average.npz"))
    tec, hours, when = g["tec"], g["hours"].astype("datetime64[h]"), g["when"].astype("datetime64[h]")
    exact = _f64_slot_means(tec, time_slots(hours))
    for series in (tec, torch.from_numpy(tec).to(dev)):                   # numpy in, device tensor in
        ha = HistoricalAverage()
        ha.fit(series, hours)
        assert isinstance(ha.averages, np.ndarray) and ha.averages.dtype == np.float64 and ha.averages.shape == (35, 12)
        print("fit: rel. error vs float64 numpy", _rel(ha.averages, exact), "vs reference", _rel(ha.averages, g["averages"]))
        assert _rel(ha.averages, exact) <= 1e-12
        assert _rel(ha.averages, g["averages"]) <= 2e-6
        pred = ha.predict(when, 35)
        assert isinstance(pred, np.ndarray) and pred.dtype == np.float64 and pred.shape == g["predict"].shape
        assert _rel(pred, exact.T[g["when_slots"]]) <= 1e-12
        assert _rel(pred, g["predict"]) <= 2e-6
    with pytest.raises(ValueError):
        ha.predict(when, 36)


def test_slot_mean_in_place_channel_empty_slot_and_determinism(dev):
    """Channel 0 of a (T, N*C) split read in place through strides, at the full grid; a series in which one slot never
    occurs gives NaN in that column and finite values elsewhere; three launches are bit-identical."""
    from src.models.baselines import slot_mean
    rng = np.random.default_rng(3)
    T, N, C = 600, 2911, 6
    X = rng.gamma(2.0, 12.0, size=(T, N, C)).astype(np.float32)
    slots = (np.arange(T) % 12).astype(np.int32)
    slots[slots == 7] = 8                                                  # slot 7 never occurs
    Xd, sd = torch.from_numpy(X).to(dev), torch.from_numpy(slots).to(dev)
    runs = [slot_mean(Xd[:, :, 0], sd, 12) for _ in range(3)]
    means, counts = runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()
    assert means.shape == (N, 12) and means.dtype == np.float64
    assert np.array_equal(counts, np.bincount(slots, minlength=12).astype(np.float64)) and counts[7] == 0
    assert np.isnan(means[:, 7]).all()
    keep = [s for s in range(12) if s != 7]
    assert np.isfinite(means[:, keep]).all()
    exact = np.stack([X[slots == s, :, 0].astype(np.float64).mean(axis=0) for s in keep], axis=1)
    assert _rel(means[:, keep], exact) <= 1e-12
    for m, c in runs[1:]:
        assert np.array_equal(m.cpu().numpy(), means, equal_nan=True) and np.array_equal(c.cpu().numpy(), counts)
    m3 = slot_mean(Xd[:, :, 3], sd, 12)[0].cpu().numpy()                   # another channel: the base pointer moves
    exact3 = np.stack([X[slots == s, :, 3].astype(np.float64).mean(axis=0) for s in keep], axis=1)
    assert _rel(m3[:, keep], exact3) <= 1e-12
    short = slot_mean(Xd[:3, :70, 0], sd[:3], 12)[0].cpu().numpy()         # T smaller than the four quarters' stride
    assert _rel(short[:, :3], X[:3, :70, 0].astype(np.float64).T) <= 1e-12 and np.isnan(short[:, 3:]).all()


def test_baseline_save_load_round_trip(dev, tmp_path):
    from src.models.baselines import HistoricalAverage, load_baseline, save_baseline
    rng = np.random.default_rng(1)
    tec = rng.gamma(2.0, 12.0, size=(240, 9)).astype(np.float32)
    hours = np.datetime64("2014-01-01T00", "h") + 2 * np.arange(240).astype("timedelta64[h]")
    ha = HistoricalAverage().fit(tec, hours)
    save_baseline(ha, str(tmp_path / "ha.joblib"))
    back = load_baseline(str(tmp_path / "ha.joblib"))
    assert np.array_equal(back.averages, ha.averages)
    assert np.array_equal(back.predict(hours[:30], 9), ha.predict(hours[:30], 9))


# ------------------------------------------------------------------------------------ evaluate_split
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


def test_evaluate_split_model_entry_equals_validate(dev, split):
    from tecmollm.evaluate import evaluate_split
    from tecmollm.loop import validate
    g, model, ds, ei, scaler = split
    res = evaluate_split(model, ds, ei, 5, scaler=scaler, baselines=("mean", "last", "periodic"))
    assert list(res) == ["TEC-MoLLM", "HistoricalAverage", "Persistence", "DayAgo"]
    for name in res:
        assert set(res[name]) == set(KEYS) and len(res[name]["mae_by_horizon"]) == 12
    _, want = validate(model, ds, ei, 5, scaler=scaler)
    _check(res["TEC-MoLLM"], want, rtol=1e-12, atol=0)
    assert list(evaluate_split(model, ds, ei, 5, scaler=scaler)) == ["TEC-MoLLM", "HistoricalAverage"]


def test_evaluate_split_historical_average_matches_the_reference(dev, split):
    """test.py:199-217 run by the reference itself on the same split, at the bars tests/test_gpu_shell.py uses for the
    metrics kernel."""
    from tecmollm.evaluate import evaluate_split
    g, model, ds, ei, scaler = split
    res = evaluate_split(model, ds, ei, 7, scaler=scaler)
    _check(res["HistoricalAverage"], {k: g[f"out_{k}"] for k in KEYS}, rtol=2e-5, atol=2e-6)


def test_stride0_baseline_view_is_read_in_place(dev, split):
    from src.evaluation.metrics import HorizonMetrics, _as_shi
    from tecmollm.evaluate import window_baseline
    g, model, ds, ei, scaler = split
    out = []
    for materialise in (False, True):
        hm = HorizonMetrics(12, scaler, device=dev)
        for a in range(0, len(ds), 6):
            chunk = list(range(a, min(a + 6, len(ds))))
            bl = window_baseline(ds, chunk, "mean")
            if materialise:
                bl = bl.contiguous()
            else:
                assert _as_shi(bl, "bl")[0].data_ptr() == bl.data_ptr() and _as_shi(bl, "bl")[5] == 0   # no copy made
            hm.update(bl, ds.batch(chunk)[2])
        out.append(hm.compute())
    _check(out[0], out[1], rtol=1e-12, atol=0)


def test_evaluate_split_order_halves_merge_to_the_full_split(dev, split):
    """order= with two disjoint halves (what two ranks' sampler shards would be): their statistics, added by hand, give
    the full split's dicts; validate(order=) takes the same argument."""
    from src.evaluation.metrics import HorizonMetrics
    from tecmollm import evaluate as E
    from tecmollm.loop import validate
    g, model, ds, ei, scaler = split
    full = E.evaluate_split(model, ds, ei, 4, scaler=scaler, baselines=("mean", "last"))
    halves = [list(range(0, len(ds), 2)), list(range(1, len(ds), 2))]
    kept = []
    orig = HorizonMetrics.compute

    def spy(self):                                                         # keep every half's statistics
        kept.append(self.stats.clone())
        return orig(self)
    HorizonMetrics.compute = spy
    try:
        for h in halves:
            E.evaluate_split(model, ds, ei, 4, scaler=scaler, baselines=("mean", "last"), order=h)
    finally:
        HorizonMetrics.compute = orig
    assert len(kept) == 6
    for i, name in enumerate(["TEC-MoLLM", "HistoricalAverage", "Persistence"]):
        hm = HorizonMetrics(12, scaler, device=dev)
        hm.stats.copy_(kept[i] + kept[3 + i])
        _check(hm.compute(), full[name], rtol=1e-12, atol=0)
    loss_a, m_a = validate(model, ds, ei, 4, scaler=scaler, order=halves[0])
    loss_f, m_f = validate(model, ds, ei, 4, scaler=scaler)
    assert m_a["mae_avg"] != m_f["mae_avg"] and np.isfinite(loss_a)

