"""GPU tests of the raw-data stage: tecm_moments against an exactly rounded fit, tecm_features_build against the fixture of
the reference's scripts/preprocess.py::main() bit for bit, tecm_window_batch_series against tecm_window_batch on the
materialised tensors, preprocess_splits end to end and SeriesWindowDataset against SlidingWindowSamplerDataset.

The kernels' own edges (csrc/preprocess.hip): the pooled moments kernel walks 256-column chunks and spreads the rows over at
most 2048 / chunks blocks, four rows at a time; the per-column kernel gives a block 256 rows and at most 256 blocks; a
thread's cascade carries after 64 and after 4096 adds.  The shapes the issue lists stay below 256 columns and below 64 adds
a thread, so MORE_POOLED / MORE_COLUMN add: 600 columns (three chunks), 2048 * 70 + 1 rows of one column (70 adds in a
block's first thread: the first carry), 2048 * 4097 + 1 rows (the second carry) and 256 * 256 * 65 + 5 rows per column (65
adds a thread in the per-column kernel)."""
import math
import os

import numpy as np
import pytest
import torch

from tests import preprocess_ref as PR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = ("train", "val", "test")
SHAPES = [(1, 1), (13, 3), (1025, 7), (4099, 15), (20000, 33)]
TAPS = (0, 1, 12, 24)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "preprocess.npz")) as z:
        return {k: z[k] for k in z.files}


def _data(rows, cols, dtype, seed=0):
    rng = np.random.default_rng(1000 * rows + cols + seed)
    x = rng.gamma(2.0, 12.0, size=(rows, cols)) + rng.normal(0.0, 1.0, size=(1, cols)) * 30.0
    return x.astype(dtype)


def _moments(x, pool, taps):
    from tecmollm.preprocess import moments
    count, mean, var = moments(x, pool=pool, taps=taps)
    return count.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy()


def _check_moments(got, want, what):
    count, mean, var = got
    for s, w in enumerate(want):
        err_m = abs(mean[s] - w[1]) / w[3] if w[3] else abs(mean[s] - w[1])
        err_v = abs(var[s] - w[2]) / w[2] if w[2] else abs(var[s] - w[2])
        print(f"{what} stat {s}: count {count[s]} mean err {err_m:.3e} var err {err_v:.3e} (bound {PR.BOUND:.0e})")
        assert count[s] == w[0], (what, s)
        assert PR.close(mean[s], var[s], w), (what, s, mean[s], var[s], w)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rows, cols", SHAPES)
def test_moments_against_an_exactly_rounded_fit(dev, rows, cols, dtype):
    x = _data(rows, cols, dtype)
    xd = torch.from_numpy(x).to(dev)
    for taps in TAPS:
        if taps >= rows:
            continue
        _check_moments(_moments(xd, True, taps), [PR.fit_exact(x, taps)], f"pooled {rows}x{cols} taps {taps}")
        _check_moments(_moments(xd, False, taps), [PR.fit_exact(x[:, c:c + 1], taps) for c in range(cols)],
                       f"columns {rows}x{cols} taps {taps}")


def _quantised(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return (np.maximum(np.round(rng.gamma(2.0, 12.0, size=(rows, cols)) * 64.0), 1.0) / 64.0).astype(np.float32)


@pytest.mark.parametrize("rows, cols, pool, taps", [(5, 600, True, 0), (30, 600, True, 12), (2048 * 70 + 1, 1, True, 12),
                                                     (2048 * 4097 + 1, 1, True, 12), (256 * 256 * 65 + 5, 2, False, 24)])
def test_moments_across_the_kernels_chunk_and_carry_edges(dev, rows, cols, pool, taps):
    x = _quantised(rows, cols, rows % 1000 + cols)
    xd = torch.from_numpy(x).to(dev)
    want = [PR.fit_exact_quantised(x, taps)] if pool else [PR.fit_exact_quantised(x[:, c:c + 1], taps) for c in range(cols)]
    _check_moments(_moments(xd, pool, taps), want, f"{'pooled' if pool else 'columns'} {rows}x{cols} taps {taps}")


def test_moments_of_a_column_slice_of_a_wider_matrix(dev):
    x = _data(1025, 9, np.float64, seed=5)
    view = torch.from_numpy(x).to(dev)[:, 1:6]                              # five columns at offset 1, ld = 9
    assert view.stride() == (9, 1) and view.data_ptr() % 16 == 8
    for taps in (0, 12):
        _check_moments(_moments(view, False, taps), [PR.fit_exact(x[:, c:c + 1], taps) for c in range(1, 6)], f"slice taps {taps}")
        _check_moments(_moments(view, True, taps), [PR.fit_exact(x[:, 1:6], taps)], f"slice pooled taps {taps}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_moments_skip_nan_and_know_a_constant_column(dev, dtype):
    from tecmollm import DeviceStandardScaler
    rows, cols = 4099, 15
    x = _data(rows, cols, dtype, seed=9)
    rng = np.random.default_rng(3)
    x[rng.random(x.shape) < 0.01] = np.nan                                 # 1 % missing
    x[:, 4] = np.nan                                                       # a column with no entry at all
    x[:, 7] = 7.3                                                          # a constant column (not exactly representable)
    xd = torch.from_numpy(x).to(dev)
    for taps in (0, 12):
        count, mean, var = _moments(xd, False, taps)
        assert count[4] == 0 and np.isnan(mean[4]) and np.isnan(var[4])
        keep = [c for c in range(cols) if c not in (4, 7)]
        _check_moments((count[keep], mean[keep], var[keep]), [PR.fit_exact(x[:, c:c + 1], taps) for c in keep], f"nan taps {taps}")
        w = PR.fit_exact(x[:, 7:8], taps)
        assert count[7] == w[0] and abs(mean[7] - w[1]) <= PR.BOUND * w[3] and PR.is_constant(var[7], mean[7], count[7])
        s = DeviceStandardScaler()._set(count, mean, var)
        assert s.scale_[7] == 1.0 and np.isnan(s.scale_[4]) and s.scale_[0] == math.sqrt(var[0])
        assert s.n_samples_seen_.tolist() == count.tolist()
        pooled = _moments(xd, True, taps)
        _check_moments(pooled, [PR.fit_exact(x, taps)], f"nan pooled taps {taps}")
    allnan = torch.full((13, 3), float("nan"), device=dev)
    count, mean, var = _moments(allnan, True, 0)
    assert count[0] == 0 and np.isnan(mean[0]) and np.isnan(var[0])


def test_moments_are_bit_reproducible(dev):
    x = torch.from_numpy(_data(20000, 33, np.float32, seed=2)).to(dev)
    for pool in (True, False):
        runs = [_moments(x, pool, 12) for _ in range(3)]
        for r in runs[1:]:
            assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(r, runs[0]))


# ------------------------------------------------------------------------------------ features build
class _Scaler:
    def __init__(self, mean, scale):
        self.mean_, self.scale_ = np.asarray(mean, dtype=np.float64).reshape(-1), np.asarray(scale, dtype=np.float64).reshape(-1)


def _scalers(golden, case):
    return (_Scaler(golden[f"{case}_scaler_mean_"], golden[f"{case}_scaler_scale_"]),
            _Scaler(golden[f"{case}_target_scaler_mean_"], golden[f"{case}_target_scaler_scale_"]))


def _same(a: torch.Tensor, b: np.ndarray) -> bool:
    a = a.cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("case", ["a", "b"])                                # a: float32 TEC, b: float64 TEC
def test_features_build_reproduces_the_fixture_bit_for_bit(dev, golden, case):
    from tecmollm.preprocess import build_features
    H = int(golden["horizon"])
    fs, ts = _scalers(golden, case)
    for s in SPLITS:
        tec, idx = golden[f"{case}_{s}_tec"], golden[f"{case}_{s}_indices"]
        T = tec.shape[0] - H
        out = build_features(tec, idx, fs, ts, horizon=H, x_rows=T, outputs=("X", "Ys", "Y"), device=dev)
        assert _same(out["X"], golden[f"{case}_{s}_X"]) and _same(out["Y"], golden[f"{case}_{s}_Y"]), (case, s)
        assert _same(out["Ys"], PR.build_ys(tec, ts.mean_[0], ts.scale_[0]))
        assert torch.equal(out["Ys"][1:T + 1], out["Y"][..., 0]) and torch.equal(out["Ys"][H:], out["Y"][..., H - 1])
        full = build_features(tec, idx.astype(np.float32), fs, ts, outputs=("X",), device=dev)["X"]       # every row, float32 indices
        assert _same(full, PR.build_x(tec, idx.astype(np.float32), fs.mean_, fs.scale_))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [1, 15, 2911])                                 # 2911 * 6 and 2911 * 2 are no multiples of 4
def test_features_build_rows_that_do_not_fill_quads(dev, N, dtype):
    from tecmollm.preprocess import build_features
    rows, H = 5, 2
    rng = np.random.default_rng(N)
    tec = rng.gamma(2.0, 12.0, size=(rows, N)).astype(dtype)
    tec[2, N // 2] = np.nan                                                # NaN in, NaN out
    idx = rng.normal(50.0, 20.0, size=(rows, 5))
    idx[3, 1] = np.nan
    fs, ts = _Scaler(rng.normal(20.0, 5.0, 6), rng.uniform(0.5, 30.0, 6)), _Scaler([23.7], [17.1])
    want = {"X": PR.build_x(tec, idx, fs.mean_, fs.scale_, rows - 1), "Ys": PR.build_ys(tec, 23.7, 17.1), "Y": PR.build_y(tec, 23.7, 17.1, H)}
    assert np.isnan(want["X"]).sum() == 1 + N and np.isnan(want["Ys"]).sum() == 1 and np.isnan(want["Y"]).sum() == 2
    out = build_features(tec, idx, fs, ts, horizon=H, x_rows=rows - 1, outputs=("X", "Ys", "Y"), device=dev)
    for k in want:
        assert _same(out[k], want[k]), k
    for leave in ("X", "Ys", "Y"):                                         # outputs left out, one at a time
        some = build_features(tec, idx, fs, ts, horizon=H, x_rows=rows - 1, outputs=[k for k in want if k != leave], device=dev)
        assert sorted(some) == sorted(k for k in want if k != leave) and all(_same(some[k], want[k]) for k in some)
    flat = torch.empty(rows * N + 1, device=dev, dtype=torch.from_numpy(tec).dtype)       # the source one element off its alignment
    flat[1:] = torch.from_numpy(tec).reshape(-1).to(dev)
    off = flat[1:].view(rows, N)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    out = build_features(off, idx, fs, ts, horizon=H, x_rows=rows - 1, outputs=("X", "Ys", "Y"), device=dev)
    for k in want:
        assert _same(out[k], want[k]), k


# ------------------------------------------------------------------------------------ window batch
def _series(T, N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(T, 1, N, 6, generator=g)
    Ys = torch.randn(T, 1, N, generator=g)
    t = torch.arange(T, dtype=torch.float32)
    tf = torch.stack([t % 12, t % 366, torch.zeros(T), (t // 30) % 4], 1)
    return X.to(dev), Ys.to(dev), tf.to(dev)


def _materialise(Ys, L_out):
    T = Ys.shape[0] - L_out
    return torch.stack([Ys[1 + h:1 + h + T] for h in range(L_out)], dim=-1).contiguous()


@pytest.mark.parametrize("N", [15, 2911])
@pytest.mark.parametrize("L_out", [1, 12, 24])
@pytest.mark.parametrize("L_in", [7, 48])
def test_window_batch_series_equals_window_batch_on_the_materialised_target(dev, L_in, L_out, N):
    from src.data.dataset import SeriesWindowDataset, SlidingWindowSamplerDataset
    T = L_in + 2 * L_out + 6
    X, Ys, tf = _series(T, N, L_in + L_out + N, dev)
    old = SlidingWindowSamplerDataset.from_tensors(X[:T - L_out], _materialise(Ys, L_out), tf[:T - L_out], L_in, L_out, device=dev)
    new = SeriesWindowDataset.from_series(X, Ys, tf, L_in, L_out, device=dev)
    assert len(new) == len(old) == 7 and new.sample_indices == old.sample_indices
    for idx in ([0], [len(old) - 1], [0, 3, 6, 1, 6]):                      # B = 1 and 5; the first and the last valid start
        for a, b in zip(new.batch(idx), old.batch(idx)):
            assert a.shape == b.shape and torch.equal(a, b)
    everything = SeriesWindowDataset.from_series(X, Ys, tf, L_in, L_out, device=dev, windows="all")
    assert len(everything) == len(new) + L_out                             # L_out more starts at stride 1
    x, _, y = everything.batch([len(everything) - 1])                      # the last start: its targets end the series
    assert torch.equal(y[0, :, :, 0], Ys[T - L_out:, 0]) and torch.equal(x[0], X[T - L_out - L_in:T - L_out, 0])
    with pytest.raises(IndexError):
        everything.batch([len(everything)])


# ------------------------------------------------------------------------------------ end to end
def _raw_splits(golden, case):
    return {s: {"tec": golden[f"{case}_{s}_tec"], "space_weather_indices": golden[f"{case}_{s}_indices"],
                "time": golden[f"{case}_{s}_time"].astype("datetime64[s]")} for s in SPLITS}


def _within_one_ulp(got: torch.Tensor, want: np.ndarray) -> bool:
    got = got.cpu().numpy()
    return got.shape == want.shape and bool((np.abs(got.astype(np.float64) - want.astype(np.float64))
                                             <= np.spacing(np.abs(want)).astype(np.float64) + 1e-11).all())


@pytest.mark.parametrize("case", ["a", "b"])
def test_preprocess_splits_end_to_end(dev, golden, case, tmp_path):
    from src.data.dataset import SeriesWindowDataset, SlidingWindowSamplerDataset
    from tecmollm import DeviceStandardScaler, preprocess_splits
    H = int(golden["horizon"])
    ref = preprocess_splits(_raw_splits(golden, case), horizon=H, output_dir=str(tmp_path / "ref"), layout="reference", device=dev)
    ser = preprocess_splits(_raw_splits(golden, case), horizon=H, output_dir=str(tmp_path / "ser"), layout="series", device=dev)
    for stem, s in (("scaler", ref.feature_scaler), ("target_scaler", ref.target_scaler)):
        n = golden[f"{case}_{stem}_n_samples_seen_"]
        assert np.array_equal(np.asarray(s.n_samples_seen_), n) and np.isscalar(s.n_samples_seen_)
        for c in range(s.mean_.size):
            col = golden[f"{case}_train_tec"] if c == 0 else golden[f"{case}_train_indices"][:-H, c - 1]
            want = (0, golden[f"{case}_{stem}_mean_"][c], golden[f"{case}_{stem}_var_"][c], float(np.abs(col).mean()))
            print(f"{case} {stem}[{c}]: mean {s.mean_[c]!r} vs {want[1]!r}, var {s.var_[c]!r} vs {want[2]!r}")
            assert PR.close(s.mean_[c], s.var_[c], want), (stem, c)
        assert np.allclose(s.scale_, golden[f"{case}_{stem}_scale_"], rtol=1e-12, atol=0)
    assert np.array_equal(ser.target_scaler.mean_, ref.target_scaler.mean_) and np.array_equal(ser.feature_scaler.var_, ref.feature_scaler.var_)
    for s in SPLITS:
        T = golden[f"{case}_{s}_tec"].shape[0] - H
        assert _within_one_ulp(ref[s]["X"], golden[f"{case}_{s}_X"]) and _within_one_ulp(ref[s]["Y"], golden[f"{case}_{s}_Y"]), (case, s)
        assert _within_one_ulp(ser[s]["X"][:T], golden[f"{case}_{s}_X"]) and ser[s]["X"].shape[0] == T + H
        assert _within_one_ulp(ser[s]["Ys"][1:T + 1], golden[f"{case}_{s}_Y"][..., 0]), (case, s)
        assert _within_one_ulp(ser[s]["Ys"][H:], golden[f"{case}_{s}_Y"][..., H - 1]) and ser[s]["horizon"] == H
        assert np.array_equal(ref[s]["time_features"].cpu().numpy(), golden[f"{case}_{s}_time_features"])
        assert np.array_equal(ser[s]["time_features"][:T].cpu().numpy(), golden[f"{case}_{s}_time_features"])
    assert sorted(os.listdir(tmp_path / "ref")) == ["scaler.joblib", "target_scaler.joblib", "test_set.pt", "train_set.pt", "val_set.pt"]
    assert sorted(os.listdir(tmp_path / "ser")) == ["scaler.joblib", "target_scaler.joblib", "test_series.pt", "train_series.pt", "val_series.pt"]
    saved = torch.load(tmp_path / "ref" / "val_set.pt")
    assert sorted(saved) == ["X", "Y", "time_features"] and all(v.dtype == torch.float32 and not v.is_cuda for v in saved.values())
    old = SlidingWindowSamplerDataset(str(tmp_path / "ref"), "val", L_in=7, L_out=H, device=dev)          # the existing loader
    assert len(old) == max(0, T_val(golden, case) - H - 7 - H + 1) and torch.equal(old.Y, ref["val"]["Y"])      # case b: too short
    new = SeriesWindowDataset(str(tmp_path / "ser"), "val", L_in=7, L_out=H, device=dev)
    direct = SeriesWindowDataset.from_preprocessed(ser, "val", L_in=7, L_out=H, device=dev)
    assert len(new) == len(direct) == len(old) and (len(old) == 10 or case == "b")
    if len(old):
        for a, b, c in zip(new.batch(range(len(new))), old.batch(range(len(old))), direct.batch(range(len(direct)))):
            assert torch.equal(a, b) and torch.equal(a, c)
    import joblib
    sk = joblib.load(tmp_path / "ser" / "target_scaler.joblib")
    host = golden[f"{case}_test_tec"].astype(np.float64).reshape(-1, 1)
    assert type(sk).__name__ == "StandardScaler" and np.array_equal(sk.transform(host), ser.target_scaler.transform(host))
    assert np.array_equal(ser.target_scaler.to_sklearn().transform(host), ser.target_scaler.transform(host))
    fed = preprocess_splits({"val": _raw_splits(golden, case)["val"]}, horizon=H, layout="reference", device=dev,
                            feature_scaler=DeviceStandardScaler(golden[f"{case}_scaler_mean_"], golden[f"{case}_scaler_var_"], golden[f"{case}_scaler_scale_"]),
                            target_scaler=DeviceStandardScaler(golden[f"{case}_target_scaler_mean_"], None, golden[f"{case}_target_scaler_scale_"]))
    assert _same(fed["val"]["X"], golden[f"{case}_val_X"]) and _same(fed["val"]["Y"], golden[f"{case}_val_Y"])        # passing scalers in skips the fit


def T_val(golden, case):
    return golden[f"{case}_val_tec"].shape[0]


# ------------------------------------------------------------------------------------ dataset
@pytest.fixture(scope="module")
def pair(dev):
    """One raw split on the 3 x 4 grid of the smallest model, preprocessed both ways."""
    from tecmollm import preprocess_splits
    rng = np.random.default_rng(31)
    T = 16 + 24 + 24 + 6
    raw = {"train": {"tec": rng.gamma(2.0, 12.0, size=(T, 3, 4)).astype(np.float32),
                     "space_weather_indices": rng.normal(50.0, 20.0, size=(T, 5)),
                     "time": np.datetime64("2015-12-28T00", "s") + 7200 * np.arange(T).astype("timedelta64[s]")}}
    return (preprocess_splits(raw, horizon=12, layout="series", device=dev), preprocess_splits(raw, horizon=12, layout="reference", device=dev), T)


def test_series_dataset_equals_the_sliding_window_dataset(dev, pair):
    from src.data.dataset import SeriesWindowDataset, SlidingWindowSamplerDataset
    ser, ref, T = pair
    for stride in (1, 3):
        old = SlidingWindowSamplerDataset.from_tensors(ref["train"]["X"], ref["train"]["Y"], ref["train"]["time_features"], 16, 12, stride, device=dev)
        new = SeriesWindowDataset.from_preprocessed(ser, "train", 16, 12, stride, device=dev)
        assert len(new) == len(old) > 0 and new.sample_indices == old.sample_indices
        assert (new.L_in, new.L_out, new.stride) == (16, 12, stride) and torch.equal(new.X, old.X) and torch.equal(new.time_features, old.time_features)
        for i in (0, len(old) - 1):
            a, b = new[i], old[i]
            assert sorted(a) == sorted(b) and all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in a)
            assert a["y"].shape == (3, 4, 12) and a["y"].data_ptr() == new.Ys[new.sample_indices[i] + 16].data_ptr()       # a view
        for a, b in zip(new.batch(range(len(new))), old.batch(range(len(old)))):
            assert torch.equal(a, b)
        with pytest.raises(IndexError):
            new[len(new)]
    with pytest.raises(AttributeError, match=r"\.Ys"):
        new.Y
    assert not hasattr(new, "Y") and new.Ys.shape == (T, 3, 4)


def test_one_series_serves_every_horizon(dev, pair):
    from src.data.dataset import SeriesWindowDataset, SlidingWindowSamplerDataset
    ser, ref, T = pair
    ds = SeriesWindowDataset.from_preprocessed(ser, "train", 16, 24, device=dev)       # preprocessed with horizon 12
    assert len(ds) == T - 24 - 16 - 24 + 1 and ds.X.shape[0] == T - 24
    x, tf, y = ds.batch([0, len(ds) - 1])
    assert y.shape == (2, 24, 12, 1)
    for b, a in enumerate((0, len(ds) - 1)):
        assert torch.equal(y[b, :, :, 0], ds.Ys[a + 16:a + 16 + 24].reshape(24, 12)) and torch.equal(x[b], ds.X[a:a + 16].reshape(16, 12, 6))
    every = SeriesWindowDataset.from_preprocessed(ser, "train", 16, 24, device=dev, windows="all")
    assert len(every) == len(ds) + 24 and every.X.shape[0] == T
    one = SeriesWindowDataset.from_preprocessed(ser, "train", 16, 1, device=dev)
    assert len(one) == T - 1 - 16 - 1 + 1
    with pytest.raises(ValueError, match="horizons"):
        SlidingWindowSamplerDataset.from_tensors(ref["train"]["X"], ref["train"]["Y"], ref["train"]["time_features"], 16, 24, device=dev)


def _identical(a, b) -> bool:
    """Two result dicts (of dicts) of floats, lists or arrays hold the same keys and the same values, bit for bit."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_identical(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_evaluation_and_validation_accept_the_series_dataset(dev, pair):
    from oracle import ref_cpu as R
    from src.data.dataset import SeriesWindowDataset, SlidingWindowSamplerDataset
    from tecmollm.evaluate import evaluate_split
    from tecmollm.loop import validate
    from tests.parity import build_model
    ser, ref, T = pair
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=12)
    model = build_model(cfg, R.init_params(cfg, seed=3), dev, "per_timestep").eval()
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev)
    old = SlidingWindowSamplerDataset.from_tensors(ref["train"]["X"], ref["train"]["Y"], ref["train"]["time_features"], 16, 12, device=dev)
    new = SeriesWindowDataset.from_preprocessed(ser, "train", 16, 12, device=dev)
    scaler = ser.target_scaler                                             # a DeviceStandardScaler where scaler= is taken
    a = evaluate_split(model, new, ei, 5, scaler=scaler, baselines=("mean", "last", "periodic"))
    b = evaluate_split(model, old, ei, 5, scaler=scaler, baselines=("mean", "last", "periodic"))
    assert _identical(a, b) and list(a) == ["TEC-MoLLM", "HistoricalAverage", "Persistence", "DayAgo"]
    la, ma = validate(model, new, ei, 5, scaler=scaler)
    lb, mb = validate(model, old, ei, 5, scaler=scaler)
    assert la == lb and _identical(ma, mb) and math.isfinite(la) and len(ma["mae_by_horizon"]) == 12
