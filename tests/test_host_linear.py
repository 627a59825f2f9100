"""LinearBaseline without a GPU: the float64 restatement (tests/linear_ref.py) against numpy's least squares, a
hand-centred ridge and a known answer; the held-out sanity property; the predictor pairs, the windows `fit` accepts and
what the library's host check refuses; the target series rebuilt from a materialised Y; pickling; the names
`tecmollm.evaluate` gives its baselines."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import linear_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tec-mollm_amd", "tecmollm", "libtecmollm_hip.so")


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return LIB


def test_linear_baseline_is_importable_with_its_defaults():
    from src.models.baselines import LinearBaseline, linear_pairs
    from tecmollm import evaluate as E
    lb = LinearBaseline(device="cpu")
    assert lb.alpha == 1.0 and lb.pooled is False and lb.coef_ is None and E.LINEAR_NAME == "Linear"
    assert linear_pairs(None, 0, (), 336) == [(0, l) for l in range(1, 49)]          # the last 48 steps
    assert linear_pairs(None, 2, (), 16) == [(2, l) for l in range(1, 17)]           # ... or all L_in of them
    assert linear_pairs([1, 12], 0, [(3, 1), (4, 2)], 16) == [(0, 1), (0, 12), (3, 1), (4, 2)]
    assert linear_pairs(None, 0, (), 336) == LR.default_pairs(336)


@pytest.mark.parametrize("kw", [
    dict(lags=range(1, 65)),                      # 64 predictors and the intercept
    dict(lags=[1, 2, 2]),                         # a pair twice
    dict(lags=[1], exog=[(0, 1)]),                # ... also through exog
    dict(lags=[0]), dict(lags=[513]), dict(lags=[1], channel=-1), dict(exog=[(1, 0)]), dict(exog=[3]),
    dict(alpha=-1.0), dict(alpha=float("nan")),
])
def test_constructor_refuses_bad_pairs_and_alpha(kw):
    from src.models.baselines import LinearBaseline
    with pytest.raises(ValueError):
        LinearBaseline(device="cpu", **kw)
    assert LinearBaseline(lags=range(1, 64), device="cpu").lags[-1] == 63            # P = 64 is served
    assert LinearBaseline(lags=[512], device="cpu").lags == [512]


def test_host_check_of_the_library_names_what_it_refuses(built_lib):
    from src.models.baselines import linear_gram_geometry as geo
    pairs = LR.default_pairs(48)
    ok = dict(pairs=pairs, T=600, N=135, Cc=6, Ty=600, L_in=48, H=12, first=0, step=1, count=541)
    tile, chunk = geo(**ok)
    assert tile >= 1 and 1 <= chunk <= 541
    assert geo(**{**ok, "count": 1}) == (tile, 1)
    for change, reason in ((dict(count=542), "targets leave"), (dict(Ty=700, T=587, count=541), "inputs leave"),
                           (dict(count=0), "count < 1"), (dict(L_in=47), "lag > L_in"), (dict(H=33), "H must"), (dict(H=0), "H must"),
                           (dict(first=-1), "first >= 0"), (dict(step=0), "step >= 1"),
                           (dict(pairs=[(6, 1)]), "channel"), (dict(pairs=[(c, 1) for c in range(9)], Cc=9), "8 distinct"),
                           (dict(pairs=[(0, 513)], L_in=600, T=2000, Ty=2000), r"\[1, 512\]")):
        with pytest.raises(ValueError, match=reason):
            geo(**{**ok, **change})
    # the limits themselves are served: P = 64, H = 32, lag 512, 8 channels, a strided progression
    geo(**{**ok, "pairs": [(0, l) for l in range(1, 64)], "L_in": 63, "H": 32, "count": 100})
    geo(**{**ok, "pairs": [(c, 512) for c in range(8)], "Cc": 8, "L_in": 512, "T": 3000, "Ty": 3000, "H": 32, "step": 3, "count": 800})
    geo(**{**ok, "pairs": []})                                               # the intercept alone


def test_restatement_equals_lstsq_at_alpha_zero_and_a_hand_centred_ridge():
    T, N, L_in, H = 400, 3, 16, 4
    rng = np.random.default_rng(3)
    X = rng.standard_normal((T, N, 3)).astype(np.float32)
    ys = LR.synthetic(T, N, 5)
    pairs = LR.default_pairs(L_in, lags=[1, 2, 5, 16], exog=[(1, 1), (2, 3)])
    first, step, count = 2, 3, 120
    starts = first + step * np.arange(count)
    z, y = LR.design(X, pairs, L_in, starts), LR.targets(ys, L_in, H, starts)
    coef, status, cond = LR.fit(X, ys, pairs, L_in, H, first, step, count, 0.0)
    assert (status == 0).all() and cond.max() < 1e4
    for n in range(N):
        want = np.linalg.lstsq(z[:, n], y[:, n], rcond=None)[0]
        assert np.abs(coef[n] - want).max() <= 1e-10
    # sklearn's Ridge(alpha, fit_intercept=True): centre, solve (Zc^T Zc + alpha I) w = Zc^T yc, intercept from the means
    alpha = 2.5
    coef, status, _ = LR.fit(X, ys, pairs, L_in, H, first, step, count, alpha)
    for n in range(N):
        zc, yc = z[:, n, 1:] - z[:, n, 1:].mean(axis=0), y[:, n] - y[:, n].mean(axis=0)
        w = np.linalg.solve(zc.T @ zc + alpha * np.eye(zc.shape[1]), zc.T @ yc)
        b = y[:, n].mean(axis=0) - z[:, n, 1:].mean(axis=0) @ w
        assert np.abs(coef[n, 1:] - w).max() <= 1e-10 and np.abs(coef[n, 0] - b).max() <= 1e-10
    # the sequential loop and the matrix products are the same sums
    a, b = LR.gram_sequential(X, ys, pairs, L_in, H, first, step, count), LR.gram(X, ys, pairs, L_in, H, first, step, count)
    assert np.abs(a - b).max() <= 1e-10 and np.array_equal(a[:, :, :len(pairs) + 1], a[:, :, :len(pairs) + 1].transpose(0, 2, 1))
    # pooled: one W from the sum of the normal equations = least squares on the stacked rows
    coef, status, _ = LR.fit(X, ys, pairs, L_in, H, first, step, count, 0.0, pool=True)
    want = np.linalg.lstsq(z.reshape(-1, z.shape[2]), y.reshape(-1, H), rcond=None)[0]
    assert coef.shape == (1, len(pairs) + 1, H) and np.abs(coef[0] - want).max() <= 1e-10


def test_restatement_recovers_a_known_map_and_marks_constant_and_nan_nodes():
    T, N, L_in, H = 300, 4, 8, 3
    rng = np.random.default_rng(11)
    X = rng.standard_normal((T, N, 2)).astype(np.float32)
    pairs = LR.default_pairs(L_in, lags=[1, 3, 8], exog=[(1, 2)])
    W = rng.standard_normal((N, len(pairs) + 1, H))
    starts = np.arange(T - L_in + 1)
    f = LR.forecast(X, pairs, L_in, starts, W)                              # (B, H, N): noiseless targets z^T W
    # one series cannot carry noiseless targets for several horizons at once (row t is horizon h of window t - L_in - h for
    # every h), so W is recovered one horizon at a time, each from a series of its own
    for h in range(H):
        ys_h = np.zeros((T + 1, N))
        ys_h[starts + L_in] = f[:, h, :]
        coef, status, _ = LR.fit(X, ys_h, pairs, L_in, 1, 0, 1, len(starts), 0.0)
        assert (status == 0).all() and np.abs(coef[:, :, 0] - W[:, :, h]).max() <= 1e-9
    # status rules
    y = LR.synthetic(T, N, 2)
    y[:, 1] = 3.25
    y[17, 2] = np.nan
    coef, status, _ = LR.fit(y[:, :, None], y, LR.default_pairs(L_in), L_in, H, 0, 1, 200, 0.0)
    assert status.tolist() == [0, LR.DEGENERATE, LR.NONFINITE, 0]
    assert np.array_equal(coef[1, 0], np.full(H, 3.25)) and (coef[1, 1:] == 0).all() and np.isnan(coef[2]).all()
    assert np.allclose(LR.forecast(y[:, :, None], LR.default_pairs(L_in), L_in, [5], coef)[0, :, 1], 3.25)


def test_held_out_sanity_property_of_the_restatement():
    """T = 600, lags 1..48, H = 12, alpha = 0, seasonal generator, 5 nodes, seed 1; fit on the first two thirds of the windows,
    score the last third: the linear forecast beats the window mean and persistence (measured: 1.04 against 1.22 and 1.63)."""
    s = LR.held_out_scores(LR.synthetic(600, 5, 1, seasonal=True))
    print(s)
    assert s["linear"] < s["mean"] and s["linear"] < s["last"]


def test_rebuilt_target_series_equals_the_series_the_materialised_y_came_from():
    from src.models.baselines import rebuilt_target_series
    T, N, L = 40, 7, 5
    ys = torch.from_numpy(LR.synthetic(T, N, 4))
    Y = torch.stack([ys[1 + h:T - L + 1 + h] for h in range(L)], dim=2)      # Y[i, :, h] = ys[i + 1 + h], (T - L, N, L)
    back = rebuilt_target_series(Y)
    assert back.shape == (T, N) and torch.isnan(back[0]).all() and torch.equal(back[1:], ys[1:])
    one = rebuilt_target_series(Y[:, :, :1])                                 # L_out = 1: nothing to append
    assert one.shape == (T - L + 1, N) and torch.equal(one[1:], ys[1:T - L + 1])


def test_fit_accepts_all_samples_or_an_arithmetic_progression_only():
    from src.models.baselines import _progression
    assert _progression(None, 10) == (0, 1, 10)
    assert _progression(range(2, 9, 3), 10) == (2, 3, 3)
    assert _progression([4], 10) == (4, 1, 1)
    assert _progression(np.arange(0, 10, 2), 10) == (0, 2, 5)
    assert _progression(list(range(6)), 10) == (0, 1, 6)
    for bad in ([0, 1, 3], [3, 2, 1], [1, 1], [], range(0), range(5, 11), [-1, 0], "abc", 3):
        with pytest.raises(ValueError):
            _progression(bad, 10)


def test_pickle_holds_numpy_only_and_forecasts_check_the_fitted_horizon():
    from src.models.baselines import LinearBaseline
    lb = LinearBaseline(lags=[1, 2], exog=[(1, 1)], alpha=0.5, device="cpu")
    lb.coef_, lb.status_ = np.zeros((3, 4, 2)), np.zeros(3, dtype=np.int32)
    lb.pairs_, lb.n_windows_, lb.L_in_, lb.H_, lb.num_nodes_ = [(0, 1), (0, 2), (1, 1)], 9, 4, 2, 3
    lb.tail_ = np.zeros((4, 3, 2), dtype=np.float32)
    lb._coef_dev = torch.zeros(4, 2, 3, dtype=torch.float64)
    state = lb.__getstate__()
    assert "_coef_dev" not in state and not any(isinstance(v, torch.Tensor) for v in state.values())
    assert isinstance(state["device"], str)
    back = pickle.loads(pickle.dumps(lb))
    assert back._coef_dev is None and np.array_equal(back.coef_, lb.coef_) and back.pairs_ == lb.pairs_
    assert back.device == torch.device("cpu") and back.alpha == 0.5 and back.H_ == 2

    class FakeDataset:
        L_in, L_out, num_samples = 4, 3, 5
    with pytest.raises(ValueError, match="horizons"):
        back.forecast_windows(FakeDataset(), [0])
    with pytest.raises(ValueError, match="before fit"):
        LinearBaseline(device="cpu").forecast_windows(FakeDataset(), [0])
    with pytest.raises(ValueError, match="before fit"):
        LinearBaseline(device="cpu").predict([0], 1)


def test_baseline_name_rules_old_and_new():
    from src.models.baselines import LinearBaseline, SarimaBaseline
    from tecmollm import evaluate as E
    assert [E.baseline_name(k) for k in ("mean", "last", "periodic")] == ["HistoricalAverage", "Persistence", "DayAgo"]
    for bad in ("sarima", "linear", "Linear", 3, None):
        with pytest.raises(ValueError, match="baselines must come from"):
            E.baseline_name(bad)
    with pytest.raises(ValueError, match="LinearBaseline given as a baseline must be fitted"):
        E.baseline_name(LinearBaseline(device="cpu"))
    with pytest.raises(ValueError, match="SarimaBaseline given as a baseline must be fitted"):
        E.baseline_name(SarimaBaseline(device="cpu"))
    lb = LinearBaseline(device="cpu")
    lb.coef_ = np.zeros((1, 2, 1))
    assert E.baseline_name(lb) == "Linear" == E.LINEAR_NAME
