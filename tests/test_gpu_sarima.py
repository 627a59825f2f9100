"""GPU tests of SarimaBaseline: the fit (tecm_sar_fit / tecm_sar_solve) and the window forecast (tecm_sar_forecast) against
the float64 numpy restatement of tests/sarima_ref.py, their edge cases, and the baseline inside tecmollm.evaluate.

Bars.  Sums (autocov, gram): 1e-12 x the sum of the absolute values of the terms, the bar of the error maps for fp64 sums
added in another order.  Coefficients and sigma^2: 1e-9 absolute, with cond(G) <= 1e3 and cond(Toeplitz gamma) <= 1e4
asserted on the restatement (relative input perturbations of 1e-13 then stay below 1e-9 through both solves).  Forecasts: one
fp32 ulp of the float64 restatement rounded to fp32, both sides using the same coefficients."""
import os

import numpy as np
import pytest
import torch

from tests import sarima_ref as SR

pytestmark = pytest.mark.gpu

CHUNK = 1024
ORDERS = {"default": ((1, 1, 1), (1, 1, 1, 12)), "ar_only": ((1, 1, 0), (1, 1, 0, 12)),
          "D_only": ((1, 0, 1), (1, 1, 1, 12)), "d_only": ((1, 1, 1), (1, 0, 1, 12))}
SIZES = (1, 63, 64, 65, 135)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


_series, _fits = {}, {}


def series(T, seed=7):
    """(T, 135) fp32, shared and never modified."""
    if (T, seed) not in _series:
        _series[(T, seed)] = SR.synthetic(T, 135, seed)
        _series[(T, seed)].setflags(write=False)
    return _series[(T, seed)]


def ref_fit(name, T):
    if (name, T) not in _fits:
        _fits[(name, T)] = SR.fit(series(T), SR.Model(*ORDERS[name]))
    return _fits[(name, T)]


def baseline(name, **kw):
    from src.models.baselines import SarimaBaseline
    return SarimaBaseline(*ORDERS[name], **kw)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------------------------ fit
@pytest.mark.parametrize("off", [-1, 0, 1])
@pytest.mark.parametrize("name", list(ORDERS))
def test_fit_matches_the_restatement(dev, name, off):
    """n = 3 chunks - 1, 3 chunks, 3 chunks + 1 (3, 3 and 4 blocks along time); N = 1, 63, 64, 65, 135; a contiguous (T, N)
    series and channel 2 of a (T, N * 6) split read in place."""
    sb, mo = baseline(name), SR.Model(*ORDERS[name])
    T = 3 * CHUNK + off + mo.o
    y, want = series(T), ref_fit(name, T)
    assert want["cond_gram"] <= 1e3 and want["cond_toeplitz"] <= 1e4, (want["cond_gram"], want["cond_toeplitz"])
    assert (want["status"] == 0).all()
    worst = {}
    for N in SIZES:
        split = torch.zeros(T, N, 6)
        split[:, :, 2] = torch.from_numpy(y[:, :N].copy())
        split = split.to(dev)
        for layout, x in (("contiguous", torch.from_numpy(y[:, :N].copy()).to(dev)), ("channel", split[:, :, 2])):
            got = host(sb.fit_device(x))
            assert (got["status"] == 0).all(), (N, layout)
            sums = {"autocov": np.abs(got["autocov"] - want["autocov"][:N]) / want["autocov_mag"][:N],
                    "gram": np.abs(got["gram"] - want["gram"][:N]) / want["gram_mag"][:N],
                    "wss": np.abs(got["wss"] - want["wss"][:N]) / want["wss"][:N]}
            diffs = {"coef": np.abs(got["coef"] - want["coef"][:N]), "sigma2": np.abs(got["sigma2"] - want["sigma2"][:N])}
            for k, v in {**sums, **diffs}.items():
                worst[k] = max(worst.get(k, 0.0), float(v.max()))
            for k, v in sums.items():
                assert v.max() <= 1e-12, (k, N, layout, v.max())
            for k, v in diffs.items():
                assert v.max() <= 1e-9, (k, N, layout, v.max())
            assert np.array_equal(got["gram"][:, :, :-1], got["gram"][:, :, :-1].transpose(0, 2, 1))
    print(name, off, "worst", worst)


def test_fit_edge_cases_constant_nan_short_and_determinism(dev):
    """A constant node is DEGENERATE with zero coefficients, a node with one NaN is NONFINITE with NaN coefficients, and
    neither changes a bit of its neighbours; a series shorter than m + Lmax + 2K steps is DEGENERATE throughout; three
    launches return the same bits."""
    sb, mo = baseline("default"), SR.Model(*ORDERS["default"])
    T = 2 * CHUNK + 40
    clean = torch.from_numpy(series(T)[:, :70].copy()).to(dev)
    dirty = clean.clone()
    dirty[:, 5] = 3.25
    dirty[1234, 64] = float("nan")
    dirty[7, 66] = float("inf")
    a, b = host(sb.fit_device(clean)), host(sb.fit_device(dirty))
    assert b["status"][5] == sb.DEGENERATE and (b["coef"][5] == 0).all() and b["sigma2"][5] == 0
    for n in (64, 66):
        assert b["status"][n] == sb.NONFINITE and np.isnan(b["coef"][n]).all() and np.isnan(b["sigma2"][n])
    keep = [n for n in range(70) if n not in (5, 64, 66)]
    for k in a:
        assert np.array_equal(a[k][keep], b[k][keep]), k
    want = SR.fit(dirty.cpu().numpy(), mo)
    assert np.array_equal(want["status"], b["status"])
    for _ in range(2):
        again = host(sb.fit_device(dirty))
        for k in b:
            assert np.array_equal(again[k], b[k], equal_nan=True), k
    need = mo.m + mo.lmax + 2 * mo.K + mo.o                               # the shortest T that is fitted
    short = host(sb.fit_device(clean[:need - 1]))
    assert (short["status"] == sb.DEGENERATE).all() and (short["coef"] == 0).all()
    assert np.allclose(short["sigma2"], short["autocov"][:, 0], rtol=0, atol=0)
    assert np.array_equal(host(sb.fit_device(clean[:need]))["status"], SR.fit(series(T)[:need, :70], mo)["status"])
    tiny = host(sb.fit_device(clean[:mo.o]))                               # nothing left after differencing
    assert (tiny["status"] == sb.DEGENERATE).all()


def test_use_ma_zero_is_the_ar_only_solve_and_fit_drops_a_non_invertible_ma(dev):
    """tecm_sar_solve with use_ma = 0 on chosen nodes equals the restatement's AR-only solve of the same Gram matrix and
    leaves the other nodes' bits alone.  The over-differenced default model on this series gives non-invertible theta on
    some nodes (asserted on the restatement): fit() ends with MA_DROPPED there and the forecasts stay finite at L_in = 336."""
    from src.models.baselines import ma_invertible
    sb, mo = baseline("default"), SR.Model(*ORDERS["default"])
    T = 3 * CHUNK + 13
    y = series(T)
    x = torch.from_numpy(y.copy()).to(dev)
    chosen = np.zeros(135, dtype=bool)
    chosen[[0, 63, 64, 100, 134]] = True
    out = sb.fit_device(x)
    before = host(out)
    sb.solve_device(x, out, torch.from_numpy((~chosen).astype(np.int8)).to(dev))
    got, want = host(out), SR.fit(y, mo, use_ma=~chosen)
    assert (got["status"][chosen] == sb.MA_DROPPED).all() and (got["status"][~chosen] == 0).all()
    assert (got["coef"][chosen][:, 3:] == 0).all()
    assert np.abs(got["coef"] - want["coef"]).max() <= 1e-9 and np.abs(got["sigma2"] - want["sigma2"]).max() <= 1e-9
    for k in got:
        assert np.array_equal(got[k][~chosen], before[k][~chosen]), k
    # fit(): the invertibility repair
    theta = ref_fit("default", T)["coef"][:, 3:]
    bad = ~SR.ma_invertible(theta, mo.ma)
    sure = np.abs(np.array([root_margin(t, mo.ma) for t in theta]) - 1.0) > 1e-6     # verdicts that 1e-9 cannot flip
    assert (bad & sure).sum() >= 3 and (~bad & sure).sum() >= 3, "the series no longer exercises both branches"
    sb.fit(x)
    assert ((sb.status_ == sb.MA_DROPPED) == bad)[sure].all()
    assert ma_invertible(sb.coef_[:, 3:], mo.ma).all() and (sb.coef_[bad & sure][:, 3:] == 0).all()
    ref = SR.fit(y, mo, use_ma=~(sb.status_ == sb.MA_DROPPED))
    assert np.abs(sb.coef_ - ref["coef"]).max() <= 1e-9
    X = x.unsqueeze(-1).contiguous()
    f = sb.forecast_series(X, [0, T - 336], 336, 24).cpu().numpy()
    assert np.isfinite(f).all() and np.abs(f).max() < 10 * np.abs(y).max()


# ------------------------------------------------------------------------------------ forecast
def root_margin(theta, lags):
    """The smallest modulus of the roots of 1 + sum theta_b z^b."""
    poly = np.zeros(max(lags) + 1)
    poly[0] = 1.0
    poly[np.asarray(lags)] = theta
    return np.abs(np.roots(poly[::-1])).min()


def ulp_check(got, want64, what):
    want = want64.astype(np.float32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    assert np.isfinite(got).all() and (err <= ulp).all(), (what, float((err / ulp).max()))
    return float((err / ulp).max())


@pytest.mark.parametrize("L_in", ["shortest", 48, 336])
@pytest.mark.parametrize("name", ["default", "D_only", "d_only"])
def test_forecast_matches_the_restatement_within_one_ulp(dev, name, L_in):
    """L_in = o + Lmax + 1 / 48 / 336, L_out = 1 / 12 / 24 (24 > s: forecasts feed the integration), B = 1 / 5, N = 135 and
    65, channel 1 of three; the output once a strided and once a permuted view.  Same coefficient tensor on both sides."""
    sb, mo = baseline(name), SR.Model(*ORDERS[name])
    L_in = mo.o + mo.lmax + 1 if L_in == "shortest" else L_in
    T = 400
    coef = ref_fit(name, 3 * CHUNK + mo.o)["coef"].copy()
    coef[~SR.ma_invertible(coef[:, len(mo.ar):], mo.ma), len(mo.ar):] = 0.0       # as fit() repairs them: e must not diverge
    y = series(T, seed=11)
    worst = 0.0
    for N in (135, 65):
        X = torch.zeros(T, N, 3)
        X[:, :, 1] = torch.from_numpy(y[:, :N].copy())
        X, cd = X.to(dev), torch.from_numpy(coef[:N].copy()).to(dev)
        for L_out in (1, 12, 24):
            for starts in ([T - L_in], [0, 7, 3, T - L_in, 1]):
                B = len(starts)
                want = np.stack([SR.forecast(y[a:a + L_in, :N], coef[:N], mo, L_out) for a in starts])
                plain = sb.forecast_series(X, starts, L_in, L_out, channel=1, coef=cd)
                assert plain.shape == (B, L_out, N) and plain.dtype == torch.float32
                worst = max(worst, ulp_check(plain.cpu().numpy(), want, (N, L_out, B)))
                wide = torch.full((B, L_out, 2 * N), -7.0, device=dev)
                sb.forecast_series(X, starts, L_in, L_out, channel=1, coef=cd, out=wide[:, :, ::2])
                perm = torch.empty(N, B, L_out, device=dev)
                sb.forecast_series(X, starts, L_in, L_out, channel=1, coef=cd, out=perm.permute(1, 2, 0))
                assert torch.equal(wide[:, :, ::2], plain) and (wide[:, :, 1::2] == -7.0).all()
                assert torch.equal(perm.permute(1, 2, 0), plain)
    print(name, L_in, "worst error in ulps", worst)


def test_forecast_edge_cases(dev):
    """Zero coefficients give the differencing rule alone (exact on trend + periodic data); NaN coefficients give NaN for
    that node only; a start outside the series that reaches the kernel gives a NaN row and the host check refuses it; a
    window shorter than o + Lmax + 1 raises ValueError, a CPU tensor TecmError; three launches return the same bits."""
    from tecmollm._lib import TecmError
    sb, mo = baseline("default"), SR.Model(*ORDERS["default"])
    T, N = 120, 70
    t = np.arange(T)
    y = (0.5 * t + (t % 12) ** 2)[:, None] + np.arange(N)[None, :]
    X = torch.from_numpy(y.astype(np.float32)).to(dev).unsqueeze(-1).contiguous()
    coef = torch.zeros(N, 6, dtype=torch.float64, device=dev)
    got = sb.forecast_series(X, [0, 10], 48, 24, coef=coef).cpu().numpy()
    assert np.array_equal(got[0], y[48:72].astype(np.float32)) and np.array_equal(got[1], y[58:82].astype(np.float32))
    ycoef = torch.from_numpy(ref_fit("default", 3 * CHUNK + 13)["coef"][:N].copy()).to(dev)
    clean = sb.forecast_series(X, [0, 10], 48, 24, coef=ycoef)
    ycoef2 = ycoef.clone()
    ycoef2[64] = float("nan")
    dirty = sb.forecast_series(X, [0, 10], 48, 24, coef=ycoef2)
    keep = [n for n in range(N) if n != 64]
    assert torch.isnan(dirty[:, :, 64]).all() and torch.equal(dirty[:, :, keep], clean[:, :, keep])
    for _ in range(2):
        assert torch.equal(sb.forecast_series(X, [0, 10], 48, 24, coef=ycoef), clean)
    far = sb.forecast_series(X, [0, T - 47, -1, 10], 48, 24, coef=ycoef, host_check=False)
    assert torch.isnan(far[1]).all() and torch.isnan(far[2]).all()
    assert torch.equal(far[0], clean[0]) and torch.equal(far[3], clean[1])
    with pytest.raises(TecmError, match="outside"):
        sb.forecast_series(X, [0, T - 47], 48, 24, coef=ycoef)
    with pytest.raises(ValueError, match="shorter"):
        sb.forecast_series(X, [0], 26, 12, coef=ycoef)
    sb.forecast_series(X, [0], 27, 12, coef=ycoef)
    with pytest.raises(TecmError):
        sb.forecast_series(X.cpu(), [0], 48, 12, coef=ycoef)
    with pytest.raises(TecmError):
        sb.fit_device(X[:, :, 0].cpu())
    with pytest.raises(TecmError):
        sb.forecast_series(X, [0], 48, 12, coef=ycoef.cpu())


# ------------------------------------------------------------------------------------ inside tecmollm.evaluate
KEYS = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg", "mae_by_horizon", "rmse_by_horizon", "r2_by_horizon",
        "pearson_by_horizon")


def _dataset(X, Y, TF, L_in, L_out, dev):
    from src.data.dataset import SlidingWindowSamplerDataset
    return SlidingWindowSamplerDataset.from_tensors(torch.as_tensor(X), torch.as_tensor(Y), torch.as_tensor(TF), L_in, L_out,
                                                    stride=1, device=dev, mode="test")


@pytest.fixture(scope="module")
def split(dev, golden_dir):
    """The small model and split of tests/test_gpu_evaluate.py, and an ARIMA(1,1,1) fitted on channel 0 of the split in place
    (T = 51: too short for the seasonal default, whose windows need 27 steps against L_in = 16)."""
    from oracle import ref_cpu as R
    from src.models.baselines import SarimaBaseline
    from tests.parity import build_model
    g = np.load(os.path.join(golden_dir, "evaluate_split.npz"))
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=12)
    model = build_model(cfg, R.init_params(cfg, seed=3), dev, "per_timestep").eval()
    ds = _dataset(g["X"], g["Y"], g["TF"], int(g["L_in"]), int(g["L_out"]), dev)
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev)
    sb = SarimaBaseline((1, 1, 1), (0, 0, 0, 0)).fit(ds.X.view(51, 12, 6)[:, :, 0])
    return g, model, ds, ei, (float(g["mean"]), float(g["scale"])), sb


def _same(a, b, exact):
    for k in KEYS:
        if exact:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        else:
            np.testing.assert_allclose(np.asarray(a[k]), np.asarray(b[k]), rtol=1e-12, atol=0, err_msg=k)


def test_sarima_is_a_baseline_of_evaluate_split_maps_ensemble_and_report(dev, split, tmp_path):
    from src.evaluation.metrics import evaluate_horizons
    from tecmollm import evaluate as E
    from tecmollm.ensemble import evaluate_ensemble
    g, model, ds, ei, scaler, sb = split
    assert (sb.status_ & (sb.DEGENERATE | sb.NONFINITE) == 0).all() and sb.coef_.shape == (12, 2)
    assert np.abs(sb.coef_ - SR.fit(g["X"][:, :, :, 0].reshape(51, 12), SR.Model((1, 1, 1), (0, 0, 0, 0)),
                                    use_ma=~(sb.status_ == sb.MA_DROPPED))["coef"]).max() <= 1e-9
    with_s = E.evaluate_split(model, ds, ei, 5, scaler=scaler, baselines=("mean", sb))
    without = E.evaluate_split(model, ds, ei, 5, scaler=scaler, baselines=("mean",))
    assert list(with_s) == ["TEC-MoLLM", "HistoricalAverage", "SARIMA"]
    for name in without:
        _same(with_s[name], without[name], exact=True)
    pred = sb.forecast_windows(ds, range(len(ds)))
    assert pred.shape == (len(ds), 12, 12, 1)
    y = ds.batch(list(range(len(ds))))[2]
    _same(with_s["SARIMA"], evaluate_horizons(y, pred, scaler), exact=False)
    assert with_s["SARIMA"]["mae_avg"] != with_s["HistoricalAverage"]["mae_avg"]
    res, maps = E.evaluate_maps(model, ds, ei, 5, scaler=scaler, baselines=("mean", sb))
    assert list(maps) == ["TEC-MoLLM", "HistoricalAverage", "SARIMA"] and maps["SARIMA"]["mae"].shape == (1, 12, 12)
    _same(res["SARIMA"], with_s["SARIMA"], exact=True)
    imp = E.improvement(with_s, baseline="SARIMA")
    assert set(imp) == {"mae", "rmse", "r2_score", "pearson_r"} and all(np.isfinite(v) for v in imp.values())
    paths = E.write_report(with_s, str(tmp_path))
    assert "SARIMA:" in open(paths["summary"]).read() and "\nSARIMA," in open(paths["csv"]).read()
    eres, emaps, _ = evaluate_ensemble(model, ds, ei, 5, members=4, seed=3, scaler=scaler, trim=1, baselines=(sb,))
    assert list(eres) == ["TEC-MoLLM", "SARIMA", "TEC-MoLLM-MC"] and "SARIMA" in emaps
    _same(eres["SARIMA"], with_s["SARIMA"], exact=True)
    with pytest.raises(ValueError, match="baselines must come from"):
        E.evaluate_split(model, ds, ei, 5, scaler=scaler, baselines=("mean", "sarima"))


def test_sarima_round_trips_through_joblib_and_predict_is_the_forecast_at_the_series_end(dev, split, tmp_path):
    from src.models.baselines import SarimaBaseline, load_baseline, save_baseline
    g, model, ds, ei, scaler, sb = split
    save_baseline(sb, str(tmp_path / "sarima.joblib"))
    back = load_baseline(str(tmp_path / "sarima.joblib"))
    assert back._coef_dev is None and np.array_equal(back.coef_, sb.coef_) and np.array_equal(back.status_, sb.status_)
    idx = [0, 5, len(ds) - 1]
    assert torch.equal(back.forecast_windows(ds, idx), sb.forecast_windows(ds, idx))
    # predict: a model fitted on the first 30 steps forecasts from step 30 on, as window 0 of a dataset with L_in = 30 does
    train = np.ascontiguousarray(g["X"][:30, :, :, 0].reshape(30, 12))
    for fitted in (SarimaBaseline((1, 1, 1), (0, 0, 0, 0)).fit(train),                        # numpy in
                   SarimaBaseline((1, 1, 1), (0, 0, 0, 0)).fit(ds.X.view(51, 12, 6)[:30, :, 0])):   # device view in
        ds30 = _dataset(g["X"], g["Y"], g["TF"], 30, 12, dev)
        want = fitted.forecast_windows(ds30, [0]).cpu().numpy()[0, :, :, 0]
        out = fitted.predict([3, 0, 11, 99], 12)
        assert sorted(out) == [0, 3, 11]
        for n, v in out.items():
            assert v.dtype == np.float64 and v.shape == (12,) and np.array_equal(v, want[:, n].astype(np.float64))
    some = SarimaBaseline((1, 1, 1), (0, 0, 0, 0)).fit(train, node_indices=[7, 2])
    assert some.coef_.shape == (2, 2) and np.array_equal(some.coef_, fitted.coef_[[7, 2]])
    both = some.predict([2, 7, 5], 12)
    assert sorted(both) == [2, 7] and np.array_equal(both[7], fitted.predict([7], 12)[7])
    with pytest.raises(ValueError):
        some.forecast_windows(ds30, [0])
