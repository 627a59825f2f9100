"""SarimaBaseline without a GPU: the lag sets and refusals of the constructor, the invertibility check, the float64
restatement (tests/sarima_ref.py) on a known answer and on a simulated AR whose coefficients it must recover, the
host-side workspace arithmetic of the library and the ABI version."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

from tests import sarima_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tec-mollm_amd", "tecmollm", "libtecmollm_hip.so")


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return LIB


def test_lag_sets_are_the_lags_of_the_expanded_product_polynomials():
    from src.models.baselines import SarimaBaseline
    for order, seasonal, ar, ma, m in (((1, 1, 1), (1, 1, 1, 12), [1, 12, 13], [1, 12, 13], 26),
                                       ((2, 0, 0), (0, 0, 0, 0), [1, 2], [], 8),
                                       ((0, 1, 1), (0, 1, 2, 12), [], [1, 12, 13, 24, 25], 50)):
        sb = SarimaBaseline(order, seasonal, device="cpu")
        mo = SR.Model(order, seasonal)
        assert sb.ar_lags.tolist() == ar == mo.ar and sb.ma_lags.tolist() == ma == mo.ma
        assert sb.long_ar == m == mo.m and sb.K == len(ar) + len(ma) and sb.offset == mo.o
    sb = SarimaBaseline(device="cpu")                                      # the reference's defaults
    assert sb.order == (1, 1, 1) and sb.seasonal_order == (1, 1, 1, 12) and sb.offset == 13 and sb.lmax == 13
    assert SarimaBaseline((1, 0, 0), (0, 0, 0, 0), long_ar=64, device="cpu").long_ar == 64


@pytest.mark.parametrize("order, seasonal, long_ar", [
    ((1, 2, 1), (1, 1, 1, 12), None),        # d outside {0, 1}
    ((1, 1, 1), (1, 2, 1, 12), None),        # D outside {0, 1}
    ((0, 1, 0), (0, 1, 0, 12), None),        # no coefficient at all
    ((3, 0, 3), (1, 0, 1, 12), None),        # K = 14 > 12
    ((1, 1, 1), (1, 1, 1, 24), None),        # Lmax = 25 is fine, ...
    ((1, 1, 1), (1, 1, 1, 32), None),        # ... Lmax = 33 is not
    ((1, 1, 1), (0, 1, 0, 64), None),        # offset 65
    ((1, 1, 1), (1, 1, 1, 0), None),         # seasonal terms without a period
    ((-1, 0, 1), (0, 0, 0, 0), None),
    ((1, 1, 1), (1, 1, 1, 12), 12),          # long AR shorter than Lmax
    ((1, 1, 1), (1, 1, 1, 12), 65),
    ((1, 1), (1, 1, 1, 12), None),
])
def test_constructor_refuses_what_the_kernels_do_not_serve(order, seasonal, long_ar):
    from src.models.baselines import SarimaBaseline
    if seasonal == (1, 1, 1, 24):
        assert SarimaBaseline(order, seasonal, device="cpu").lmax == 25
        return
    with pytest.raises(ValueError):
        SarimaBaseline(order, seasonal, long_ar=long_ar, device="cpu")


def test_invertibility_check_on_hand_polynomials():
    from src.models.baselines import ma_invertible
    for fn in (ma_invertible, SR.ma_invertible):
        assert fn(np.array([[0.5], [-0.5], [1.5], [-1.5], [np.nan]]), [1]).tolist() == [True, True, False, False, True]
        # 1 + 0.5 z^12: roots at |z| = 2^(1/12) > 1;  1 + 2 z^12: inside.  (1 + 0.5 z)(1 + 0.5 z^12) expanded: invertible.
        assert fn(np.array([[0.5], [2.0]]), [12]).tolist() == [True, False]
        assert fn(np.array([[0.5, 0.5, 0.25], [1.5, 0.5, 0.75], [0.5, 1.5, 0.75]]), [1, 12, 13]).tolist() == [True, False, False]
        assert fn(np.zeros((3, 0)), []).tolist() == [True, True, True]
    rng = np.random.default_rng(0)
    theta = rng.uniform(-1.2, 1.2, (200, 3))
    assert ma_invertible(theta, [1, 12, 13]).tolist() == SR.ma_invertible(theta, [1, 12, 13]).tolist()


def test_zero_coefficients_continue_a_trend_plus_seasonal_series_exactly():
    """coef = 0 with d = D = 1: the forecast is the differencing rule alone, which reproduces 0.5 t + (t mod 12)^2 -- linear
    trend plus an exactly periodic part -- without error; horizons past s feed on earlier forecasts."""
    mo = SR.Model()
    t = np.arange(48 + 30)
    y = (0.5 * t + (t % 12) ** 2)[:, None].repeat(2, axis=1)
    got = SR.forecast(y[:48], np.zeros((2, mo.K)), mo, 30)
    assert np.abs(got - y[48:]).max() == 0.0
    for d, D in ((1, 0), (0, 1)):                                       # d alone continues a constant, D alone a periodic series
        mo = SR.Model((1, d, 0), (0, D, 0, 12))
        y = ((t % 12) ** 2 if D else np.full(t.shape, 3.0))[:, None]
        assert np.abs(SR.forecast(y[:48], np.zeros((1, 1)), mo, 30) - y[48:]).max() == 0.0


def test_restatement_recovers_a_simulated_subset_ar():
    """w_t = 0.6 w_{t-1} + 0.5 w_{t-12} - 0.3 w_{t-13} + e_t, T = 4000, seeds 0..7, fitted as the pure AR over lags {1, 12, 13}
    of the undifferenced series: every coefficient within 4 / sqrt(T) = 0.063 of the truth (four asymptotic standard errors of
    a unit-variance regressor; worst seen 0.026)."""
    T, truth = 4000, np.array([0.6, 0.5, -0.3])
    w = np.zeros((T + 500, 8))
    for seed in range(8):
        e = np.random.default_rng(seed).standard_normal(T + 500)
        for t in range(13, T + 500):
            w[t, seed] = 0.6 * w[t - 1, seed] + 0.5 * w[t - 12, seed] - 0.3 * w[t - 13, seed] + e[t]
    mo = SR.Model((1, 0, 0), (1, 0, 0, 12))
    assert mo.ar == [1, 12, 13] and mo.ma == []
    res = SR.fit(w[500:], mo)
    assert (res["status"] == 0).all()
    err = np.abs(res["coef"] - truth).max()
    print("worst coefficient error", err)
    assert err <= 4 / np.sqrt(T)
    assert np.abs(res["sigma2"] - 1.0).max() < 0.1


def test_restatement_flags_degenerate_and_nonfinite_nodes():
    y = SR.synthetic(600, 4, seed=1)
    y[:, 1] = 7.0
    y[300, 2] = np.nan
    mo = SR.Model()
    res = SR.fit(y, mo)
    assert res["status"].tolist() == [0, SR.DEGENERATE, SR.NONFINITE, 0]
    assert (res["coef"][1] == 0).all() and np.isnan(res["coef"][2]).all() and np.isfinite(res["coef"][[0, 3]]).all()
    assert (SR.fit(y[:63], mo)["status"][[0, 3]] == SR.DEGENERATE).all()           # n = 50 < 26 + 13 + 12
    assert (SR.fit(y[:64], mo)["status"][[0, 3]] == 0).all()
    dropped = SR.fit(y, mo, use_ma=np.array([1, 1, 1, 0]))
    assert dropped["status"].tolist() == [0, SR.DEGENERATE, SR.NONFINITE, SR.MA_DROPPED]
    assert (dropped["coef"][3, 3:] == 0).all() and np.array_equal(dropped["coef"][0], res["coef"][0])


def test_workspace_bytes_are_host_arithmetic(built_lib):
    """tecm_sar_fit_ws_bytes needs no GPU: per padded node (64 per tile) and chunk of 1024 steps, m + 1 autocovariance and
    91 Gram partials, plus the m + 1 joined autocovariances and the m long-AR coefficients."""
    from tecmollm import _lib
    from src.models.baselines import _lag_array
    h = _lib.lib()

    def nbytes(T, N, m=26, d=1, D=1, s=12, ar=(1, 12, 13), ma=(1, 12, 13)):
        f = _lib.TecmSarFit(T=T, N=N, d=d, D=D, s=s, m=m, n_ar=len(ar), n_ma=len(ma), ar_lags=_lag_array(ar), ma_lags=_lag_array(ma))
        return h.tecm_sar_fit_ws_bytes(C.byref(f))
    for T, N, chunks, npad in ((1024 + 13, 1, 1, 64), (1024 + 14, 65, 2, 128), (26000, 2911, 26, 2944), (5, 64, 1, 64)):
        assert nbytes(T, N) == 8 * npad * (chunks * 27 + 27 + 26 + chunks * 91), (T, N)
    assert nbytes(3000, 64, m=8, d=0, D=0, s=0, ar=(1, 2), ma=()) == 8 * 64 * (3 * 9 + 9 + 8 + 3 * 91)
    assert nbytes(3000, 64, m=12) == -1 and b"long AR" in h.tecm_last_error()              # m < Lmax
    assert nbytes(3000, 64, ar=(12, 1, 13)) == -1 and nbytes(3000, 64, ar=(1, 12, 33)) == -1
    assert nbytes(3000, 64, d=2) == -1 and nbytes(3000, 0) == -1 and nbytes(3000, 64, D=1, s=64) == -1


def test_abi_version_is_unchanged_and_the_header_cites_the_reference(built_lib):
    from tecmollm import _lib
    header = open(os.path.join(ROOT, "include", "tecmollm.h")).read()
    assert _lib.ABI_VERSION == 21 == int(re.search(r"#define\s+TECM_ABI_VERSION\s+(\d+)", header).group(1))
    assert _lib.lib().tecm_abi_version() == 21
    for name in ("tecm_sar_fit_ws_bytes", "tecm_sar_fit", "tecm_sar_solve", "tecm_sar_forecast"):
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\s*\(", header)
    assert header.count("src/models/baselines.py:47-72") >= 1 and "src/models/baselines.py:64-72" in header
    assert C.sizeof(_lib.TecmSarForecast) == C.sizeof(_lib.TecmWindowBaseline) + 8 + 6 * 4 + 2 * 48
    for c in ("TECM_SAR_MAX_K", "TECM_SAR_MAX_LAG", "TECM_SAR_MAX_LONG_AR", "TECM_SAR_MAX_OFFSET", "TECM_SAR_CHUNK",
              "TECM_SAR_DEGENERATE", "TECM_SAR_NONFINITE", "TECM_SAR_MA_DROPPED"):
        assert int(re.search(rf"\b{c}\s*=\s*(\d+)", header).group(1)) == getattr(_lib, c), c


def test_unfitted_and_pickled_state_is_numpy_only():
    from src.models.baselines import SarimaBaseline
    sb = SarimaBaseline(device="cpu")
    with pytest.raises(ValueError):
        sb.predict([0], 12)
    sb.coef_, sb.nodes_ = np.zeros((2, 6)), np.arange(2)
    back = pickle.loads(pickle.dumps(sb))
    assert back.ar_lags.tolist() == [1, 12, 13] and back._coef_dev is None and str(back.device) == "cpu"
    assert all(not hasattr(v, "is_cuda") or k == "device" for k, v in back.__dict__.items())


def test_evaluate_names_a_fitted_sarima_and_still_refuses_unknown_strings():
    from src.models.baselines import SarimaBaseline
    from tecmollm import evaluate as E
    sb = SarimaBaseline(device="cpu")
    with pytest.raises(ValueError, match="must be fitted"):
        E.baseline_name(sb)
    sb.coef_ = np.zeros((2, 6))
    assert E.baseline_name(sb) == "SARIMA" and E.baseline_name("mean") == "HistoricalAverage"
    for bad in ("sarima", 3, None):
        with pytest.raises(ValueError, match="baselines must come from"):
            E.baseline_name(bad)
