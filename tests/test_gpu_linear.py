"""GPU tests of LinearBaseline: the normal equations (tecm_lin_gram), their solve (tecm_lin_solve) and the window forecast
(tecm_lin_forecast) against the float64 numpy restatement of tests/linear_ref.py, and the baseline inside tecmollm.evaluate.

Bars.  Gram: the bits of the sequential restatement (one running fp64 sum per entry, exact products).  Coefficients: 1e-9
absolute with cond(G + alpha D) <= 1e4 asserted on the restatement (relative perturbations of 1e-14 from the elimination order
then stay below 1e-9), and the normal-equation residual <= 1e-12 (|G| |W| + |R|) in the infinity norm with no condition cap
(Cholesky is backward stable: P eps is 7e-15 at P = 64).  Forecasts: one fp32 ulp of the float64 restatement rounded to fp32,
both sides using the device's coefficients."""
import numpy as np
import pytest
import torch

from tests import linear_ref as LR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def geometry(pairs, Cc, L_in, H, step):
    """(nodes per block, windows per staged chunk) the host picks for this shape, the chunk not capped by a window count."""
    from src.models.baselines import linear_gram_geometry
    return linear_gram_geometry(pairs, 1 << 40, 135, Cc, 1 << 40, L_in, H, 0, step, 1 << 20)


_splits = {}


def split(rows, N, Cc, H, seed):
    """X (rows, N, Cc) and ys (rows + H, N) fp32, shared and never modified: channel 0 is an AR(1), the others white."""
    key = (rows, N, Cc, H, seed)
    if key not in _splits:
        X = np.random.default_rng(seed).standard_normal((rows, N, Cc)).astype(np.float32)
        X[:, :, 0] = LR.synthetic(rows, N, seed)
        ys = LR.synthetic(rows + H, N, seed + 1, seasonal=True)
        X.setflags(write=False)
        ys.setflags(write=False)
        _splits[key] = (X, ys)
    return _splits[key]


def device_gram(dev, X, ys, pairs, L_in, H, first, step, count, pooled=False, strided=False):
    from src.models.baselines import linear_gram
    Xd = torch.tensor(X).to(dev)                            # torch.tensor copies: the shared arrays stay read-only
    if strided:                                             # ys as column 1 of a (Ty, N, 2) tensor: stride_n = 2
        wide = torch.full(ys.shape + (2,), 7.0)
        wide[:, :, 1] = torch.tensor(ys)
        yd = wide.to(dev)[:, :, 1]
    else:
        yd = torch.tensor(ys).to(dev)
    g, gp = linear_gram(Xd, yd, pairs, L_in, H, first, step, count, pooled)
    torch.cuda.synchronize()
    return g.cpu().numpy(), None if gp is None else gp.cpu().numpy()


def symmetric(g):
    P = g.shape[1]
    return np.array_equal(g[:, :, :P], g[:, :, :P].transpose(0, 2, 1))


# ------------------------------------------------------------------------------------ gram
def test_gram_default_shape_either_side_of_a_chunk_boundary_and_across_three_chunks(dev):
    """P = 49, H = 12 (P + H = 61), C = 1, stride-1 windows from row 0, tile + 1 nodes (two blocks, the second with one live
    node): chunk - 1, chunk, chunk + 1 and 2 chunk + 3 windows."""
    L_in, H = 48, 12
    pairs = LR.default_pairs(L_in)
    tile, chunk = geometry(pairs, 1, L_in, H, 1)
    counts = (chunk - 1, chunk, chunk + 1, 2 * chunk + 3)
    X, ys = split(counts[-1] - 1 + L_in, tile + 1, 1, H, 3)
    want = LR.gram_sequential(X, ys, pairs, L_in, H, 0, 1, counts[-1], snapshots=counts)
    for count in counts:
        got, _ = device_gram(dev, X, ys, pairs, L_in, H, 0, 1, count)
        assert np.array_equal(got, want[count]), (count, np.abs(got - want[count]).max())
        assert symmetric(got)


def test_gram_exogenous_channels_strided_windows_every_node_count(dev):
    """C = 6 with predictors on five channels, non-contiguous look-backs whose largest equals L_in, H = 32, first = 3, step = 3,
    ys once contiguous and once a strided view; N = 1, tile - 1, tile, tile + 1, 135 across three chunks, and the window counts
    around the chunk boundary at tile + 1 nodes."""
    L_in, H, first, step = 48, 32, 3, 3
    pairs = LR.default_pairs(L_in, lags=[1, 2, 3, 5, 8, 13, 24, 48], exog=[(1, 1), (2, 2), (3, 1), (5, 48)])
    tile, chunk = geometry(pairs, 6, L_in, H, step)
    counts = (chunk - 1, chunk, chunk + 1, 2 * chunk + 1)
    X, ys = split(first + (counts[-1] - 1) * step + L_in, 135, 6, H, 5)
    want = LR.gram_sequential(X, ys, pairs, L_in, H, first, step, counts[-1], snapshots=counts)
    for N in sorted({1, tile - 1, tile, tile + 1, 135} - {0}):
        for strided in (False, True):
            got, _ = device_gram(dev, X[:, :N], ys[:, :N], pairs, L_in, H, first, step, counts[-1], strided=strided)
            assert np.array_equal(got, want[counts[-1]][:N]), (N, strided)
            assert symmetric(got)
    for count in counts[:-1]:
        got, _ = device_gram(dev, X[:, :tile + 1], ys[:, :tile + 1], pairs, L_in, H, first, step, count, strided=True)
        assert np.array_equal(got, want[count][:tile + 1]), count


@pytest.mark.parametrize("P, H", [(1, 12), (2, 1), (33, 31), (49, 15), (49, 16), (64, 1), (64, 32)])
def test_gram_every_rectangle_shape(dev, P, H):
    """P = 1 (the intercept alone), 2, 49, 64; H = 1, 12, 32; P + H = 64 and 65; steps 1 and 3 from first = 1; 3 nodes."""
    L_in = max(P - 1, 4)
    pairs = LR.default_pairs(L_in, lags=range(1, P))
    for step in (1, 3):
        X, ys = split(1 + 39 * step + L_in, 3, 1, H, 7)
        want = LR.gram_sequential(X, ys, pairs, L_in, H, 1, step, 40)
        got, _ = device_gram(dev, X, ys, pairs, L_in, H, 1, step, 40)
        assert got.shape == (3, P, P + H) and np.array_equal(got, want) and symmetric(got), (P, H, step)


def test_gram_is_reproducible_pooled_is_the_ascending_node_sum_and_a_nan_marks_its_node_only(dev):
    from src.models.baselines import LinearBaseline, linear_solve
    L_in, H = 16, 12
    pairs = LR.default_pairs(L_in, exog=[(2, 4)])
    X, ys = split(300, 70, 3, H, 9)
    count = 300 - L_in + 1
    got, pooled = device_gram(dev, X, ys, pairs, L_in, H, 0, 1, count, pooled=True)
    assert np.array_equal(got, LR.gram_sequential(X, ys, pairs, L_in, H, 0, 1, count))
    assert np.array_equal(pooled, LR.pooled(got))
    for _ in range(2):
        again, pooled2 = device_gram(dev, X, ys, pairs, L_in, H, 0, 1, count, pooled=True)
        assert np.array_equal(again, got) and np.array_equal(pooled2, pooled)
    dirty_x, dirty_y = X.copy(), ys.copy()
    dirty_x[123, 5, 0] = np.nan                             # a predictor of node 5
    dirty_y[200, 64] = np.inf                               # a target of node 64
    dirty_x[50, 7, 1] = np.nan                              # channel 1 is no predictor: node 7 stays clean
    bad, bad_pooled = device_gram(dev, dirty_x, dirty_y, pairs, L_in, H, 0, 1, count, pooled=True)
    keep = [n for n in range(70) if n not in (5, 64)]
    assert np.array_equal(bad[keep], got[keep]) and not np.isfinite(bad[5]).all() and not np.isfinite(bad[64]).all()
    assert not np.isfinite(bad_pooled).all()
    coef, coef_t, status = linear_solve(torch.from_numpy(bad).to(dev), 1.0)
    clean = linear_solve(torch.from_numpy(got).to(dev), 1.0)[0].cpu().numpy()
    coef, status = coef.cpu().numpy(), status.cpu().numpy()
    assert (status[keep] == 0).all() and status[5] == status[64] == LinearBaseline.NONFINITE
    assert np.isnan(coef[5]).all() and np.isnan(coef[64]).all() and np.array_equal(coef[keep], clean[keep])
    assert torch.equal(coef_t.cpu()[:, :, keep], torch.from_numpy(clean).permute(1, 2, 0)[:, :, keep])


def test_host_refusals_reach_python_as_value_errors(dev):
    from src.models.baselines import linear_gram
    from tecmollm._lib import TecmError
    X, ys = split(300, 70, 3, 12, 9)
    Xd, yd = torch.from_numpy(X.copy()).to(dev), torch.from_numpy(ys.copy()).to(dev)
    pairs = LR.default_pairs(16)
    for kw, reason in ((dict(count=286), "inputs leave"), (dict(count=0), "count < 1"), (dict(L_in=15), "lag > L_in"),
                       (dict(first=-1), "first >= 0")):
        args = {**dict(L_in=16, H=12, first=0, step=1, count=285), **kw}
        with pytest.raises(ValueError, match=reason):
            linear_gram(Xd, yd, pairs, **args)
    with pytest.raises(ValueError, match="targets leave"):
        linear_gram(Xd, yd[:299], pairs, 16, 12, 0, 1, 285)
    with pytest.raises(TecmError):
        linear_gram(Xd.cpu(), yd, pairs, 16, 12, 0, 1, 285)


# ------------------------------------------------------------------------------------ solve
def norm_inf(a):
    return np.abs(a).sum(axis=-1).max(axis=-1)


def residual_check(g, coef, alpha, what):
    P = g.shape[1]
    A, R = LR.ridge_matrix(g, alpha), g[:, :, P:]
    res = norm_inf(A @ coef - R)
    bound = 1e-12 * (norm_inf(g[:, :, :P]) * norm_inf(coef) + norm_inf(R))
    worst = float((res / np.maximum(bound, np.finfo(np.float64).tiny)).max())     # an all-zero system has bound = residual = 0
    assert (res <= bound).all(), (what, worst)
    return worst


@pytest.mark.parametrize("phi, alpha, seasonal", [(0.5, 0.0, False), (0.9, 1.0, False), (0.5, 0.0, True), (0.99, 0.0, False)])
def test_solve_matches_the_restatement_and_the_normal_equations(dev, phi, alpha, seasonal):
    """Lags 1..48, H = 12, 600 windows, 8 nodes, per node and pooled.  Up to phi = 0.9 the systems are well conditioned
    (asserted <= 1e4 on the restatement) and carry the 1e-9 bar; phi = 0.99 at alpha = 0 is not and carries the residual
    bar alone, as every case does."""
    from src.models.baselines import linear_solve
    L_in, H, count = 48, 12, 600
    pairs = LR.default_pairs(L_in)
    y = LR.synthetic(count - 1 + L_in + H, 8, 7, seasonal=seasonal, phi=phi)
    g, gp = device_gram(dev, y[:-H, :, None], y, pairs, L_in, H, 0, 1, count, pooled=True)
    for gram, n_sys in ((g, 8), (gp[None], 1)):
        coef, coef_t, status = linear_solve(torch.from_numpy(np.ascontiguousarray(gram)).to(dev), alpha)
        coef, coef_t, status = coef.cpu().numpy(), coef_t.cpu().numpy(), status.cpu().numpy()
        assert coef.shape == (n_sys, 49, H) and (status == 0).all() and np.array_equal(coef_t, coef.transpose(1, 2, 0))
        want, want_status, cond = LR.solve(gram, alpha)
        assert (want_status == 0).all()
        worst = residual_check(gram, coef, alpha, (phi, alpha, seasonal, n_sys))
        print(phi, alpha, seasonal, n_sys, "cond", cond.max(), "coef error", np.abs(coef - want).max(), "residual / bound", worst)
        if phi <= 0.9:
            assert cond.max() <= 1e4, cond.max()
            assert np.abs(coef - want).max() <= 1e-9


def test_solve_constant_series_is_degenerate_with_the_mean_target_fallback(dev):
    from src.models.baselines import LinearBaseline, linear_solve
    L_in, H, count = 8, 3, 200
    pairs = LR.default_pairs(L_in)
    y = LR.synthetic(count - 1 + L_in + H, 6, 2).copy()
    clean, _ = device_gram(dev, y[:-H, :, None], y, pairs, L_in, H, 0, 1, count)
    y[:, 1] = 3.25
    y[:, 4] = 0.0
    g, _ = device_gram(dev, y[:-H, :, None], y, pairs, L_in, H, 0, 1, count)
    coef, _, status = linear_solve(torch.from_numpy(g).to(dev), 0.0)
    coef, status = coef.cpu().numpy(), status.cpu().numpy()
    want, want_status, _ = LR.solve(g, 0.0)
    assert status.tolist() == want_status.tolist() == [0, LinearBaseline.DEGENERATE, 0, 0, LinearBaseline.DEGENERATE, 0]
    assert np.array_equal(coef[1, 0], np.full(H, 3.25)) and (coef[1, 1:] == 0).all() and (coef[4] == 0).all()
    keep = [0, 2, 3, 5]
    assert np.array_equal(coef[keep], linear_solve(torch.from_numpy(clean).to(dev), 0.0)[0].cpu().numpy()[keep])
    assert np.abs(coef[keep] - want[keep]).max() <= 1e-9
    # with alpha > 0 the ridge term lifts every pivot but the intercept's: the same series is solved, with zero slopes
    coef, _, status = linear_solve(torch.from_numpy(g).to(dev), 1.0)
    coef = coef.cpu().numpy()
    assert (status.cpu().numpy() == 0).all() and np.abs(coef[1, 0] - 3.25).max() <= 1e-9 and np.abs(coef[1, 1:]).max() <= 1e-9
    residual_check(g, coef, 1.0, "constant nodes with a ridge term")


# ------------------------------------------------------------------------------------ forecast
def ulp_check(got, want64, what):
    want = want64.astype(np.float32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    assert np.isfinite(got).all() and (err <= ulp).all(), (what, float((err / ulp).max()))
    return float((err / ulp).max())


@pytest.mark.parametrize("H", [1, 12, 13, 32])
def test_forecast_matches_the_restatement_within_one_ulp(dev, H):
    """L_in = 48, default lags plus two exogenous pairs on a three-channel split; H = 1, 12, 13, 32 (every accumulator count
    the kernel is built for); B = 1 and 5; N = 135 and 65; the output plain, strided and permuted; per-node and pooled
    coefficients (stride 0), each taken from the device on both sides."""
    from src.models.baselines import LinearBaseline
    L_in, T = 48, 400
    X, ys = split(T, 135, 3, H, 13)
    worst = 0.0
    for pooled in (False, True):
        lb = LinearBaseline(exog=[(1, 1), (2, 5)], alpha=1.0, pooled=pooled, device=dev)
        lb.fit_series(torch.from_numpy(X.copy()).to(dev), torch.from_numpy(ys.copy()).to(dev), L_in, H, 0, 1, T - L_in + 1)
        assert lb.coef_.shape == ((1 if pooled else 135), 51, H) and (lb.status_ == 0).all() and lb.n_windows_ == T - L_in + 1
        full = lb._coef_on(dev)
        assert full.shape == ((51, H) if pooled else (51, H, 135))
        for N in (135, 65):
            Xd = torch.tensor(X[:, :N]).to(dev)
            cd = full if pooled else full[:, :, :N].contiguous()
            cn = lb.coef_ if pooled else lb.coef_[:N]
            for starts in ([T - L_in], [0, 7, 3, T - L_in, 1]):
                B = len(starts)
                want = LR.forecast(X[:, :N], lb.pairs_, L_in, starts, cn)
                plain = lb.forecast_series(Xd, starts, L_in, H, coef=cd)
                assert plain.shape == (B, H, N) and plain.dtype == torch.float32
                worst = max(worst, ulp_check(plain.cpu().numpy(), want, (pooled, N, B)))
                wide = torch.full((B, H, 2 * N), -7.0, device=dev)
                lb.forecast_series(Xd, starts, L_in, H, coef=cd, out=wide[:, :, ::2])
                perm = torch.empty(N, B, H, device=dev)
                lb.forecast_series(Xd, starts, L_in, H, coef=cd, out=perm.permute(1, 2, 0))
                assert torch.equal(wide[:, :, ::2], plain) and (wide[:, :, 1::2] == -7.0).all()
                assert torch.equal(perm.permute(1, 2, 0), plain)
    print(H, "worst error in ulps", worst)


def test_forecast_edge_cases(dev):
    """A start outside the series that reaches the kernel gives a NaN row and the host check refuses it; NaN coefficients give
    NaN for that node only; another L_out than the fitted one raises ValueError; three launches return the same bits."""
    from src.models.baselines import LinearBaseline
    from tecmollm._lib import TecmError
    L_in, H, T, N = 48, 12, 120, 70
    X, ys = split(T, N, 3, H, 17)
    Xd = torch.from_numpy(X.copy()).to(dev)
    lb = LinearBaseline(exog=[(1, 48)], device=dev).fit_series(Xd, torch.from_numpy(ys.copy()).to(dev), L_in, H, 0, 1, T - L_in + 1)
    clean = lb.forecast_series(Xd, [0, 10], L_in, H)
    for _ in range(2):
        assert torch.equal(lb.forecast_series(Xd, [0, 10], L_in, H), clean)
    far = lb.forecast_series(Xd, [0, T - 47, -1, 10], L_in, H, host_check=False)
    assert torch.isnan(far[1]).all() and torch.isnan(far[2]).all()
    assert torch.equal(far[0], clean[0]) and torch.equal(far[3], clean[1])
    with pytest.raises(TecmError, match="outside"):
        lb.forecast_series(Xd, [0, T - 47], L_in, H)
    lb.forecast_series(Xd, [T - 48], L_in, H)                # the last window is inside
    coef = lb._coef_on(dev).clone()
    coef[:, :, 64] = float("nan")
    dirty = lb.forecast_series(Xd, [0, 10], L_in, H, coef=coef)
    keep = [n for n in range(N) if n != 64]
    assert torch.isnan(dirty[:, :, 64]).all() and torch.equal(dirty[:, :, keep], clean[:, :, keep])
    with pytest.raises(ValueError, match="horizons"):
        lb.forecast_series(Xd, [0], L_in, 6)
    with pytest.raises(TecmError):
        lb.forecast_series(Xd.cpu(), [0], L_in, H)
    with pytest.raises(TecmError, match="lag > L_in"):
        lb.forecast_series(Xd, [0], 47, H)


# ------------------------------------------------------------------------------------ inside tecmollm.evaluate
KEYS = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg", "mae_by_horizon", "rmse_by_horizon", "r2_by_horizon",
        "pearson_by_horizon")
L_IN, L_OUT, T_ALL = 48, 12, 600


def _same(a, b, exact):
    for k in KEYS:
        if exact:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        else:
            np.testing.assert_allclose(np.asarray(a[k]), np.asarray(b[k]), rtol=1e-12, atol=0, err_msg=k)


@pytest.fixture(scope="module")
def world(dev):
    """A 12-node model and a split of its own: 600 steps of the seasonal generator (seed 1) as channel 0 of X and as the
    target series, so that the window baselines and the targets share a scale.  `full` holds every window, `test` the last
    third of them (rows 360 on), and the linear baseline is fitted on the first two thirds."""
    from oracle import ref_cpu as R
    from src.data.dataset import SeriesWindowDataset
    from src.models.baselines import LinearBaseline
    from tests.parity import build_model
    rng = np.random.default_rng(21)
    y = LR.synthetic(T_ALL, 12, 1, seasonal=True)
    X = rng.standard_normal((T_ALL, 3, 4, 6)).astype(np.float32)
    X[:, :, :, 0] = y.reshape(T_ALL, 3, 4)
    TF = np.stack([rng.integers(0, 12, T_ALL), rng.integers(0, 366, T_ALL), rng.integers(0, 13, T_ALL),
                   rng.integers(0, 4, T_ALL)], axis=1).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    full = SeriesWindowDataset.from_series(t(X), t(y.reshape(T_ALL, 3, 4)), t(TF), L_IN, L_OUT, device=dev, mode="test", windows="all")
    S = len(full)
    n_fit = 2 * S // 3
    test = SeriesWindowDataset.from_series(t(X[n_fit:]), t(y[n_fit:].reshape(-1, 3, 4)), t(TF[n_fit:]), L_IN, L_OUT, device=dev,
                                           mode="test", windows="all")
    assert S == T_ALL - L_IN - L_OUT + 1 and len(test) == S - n_fit
    cfg = R.default_config(L_in=L_IN, L_out=L_OUT, num_nodes=12)
    model = build_model(cfg, R.init_params(cfg, seed=3), dev, "per_timestep").eval()
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev)
    lin = LinearBaseline(alpha=0.0, device=dev).fit(full, range(n_fit))
    return dict(X=X, y=y, TF=TF, full=full, test=test, n_fit=n_fit, model=model, ei=ei, scaler=(20.0, 7.0), lin=lin)


def test_fit_equals_the_restatement_and_beats_window_mean_and_persistence_on_held_out_windows(dev, world):
    from tecmollm import evaluate as E
    full, lin, n_fit, y = world["full"], world["lin"], world["n_fit"], world["y"]
    X3 = world["X"].reshape(T_ALL, 12, 6)
    want, status, cond = LR.fit(X3, y, LR.default_pairs(L_IN), L_IN, L_OUT, 0, 1, n_fit, 0.0)
    assert lin.coef_.shape == (12, 49, L_OUT) and lin.coef_.dtype == np.float64 and (lin.status_ == 0).all()
    assert lin.pairs_ == LR.default_pairs(L_IN) and lin.n_windows_ == n_fit
    assert cond.max() <= 1e4 and np.abs(lin.coef_ - want).max() <= 1e-9
    held = list(range(n_fit, len(full)))
    truth = full.batch(held)[2].double()
    score = lambda pred: float(((pred.double() - truth) ** 2).mean().sqrt())
    s = {"linear": score(lin.forecast_windows(full, held)), "mean": score(E.window_baseline(full, held, "mean")),
         "last": score(E.window_baseline(full, held, "last"))}
    ref = LR.held_out_scores(y)
    print(s, ref)
    assert s["linear"] < s["mean"] and s["linear"] < s["last"]
    for k in s:
        assert abs(s[k] - ref[k]) <= 1e-5 * ref[k], k


def test_linear_is_a_baseline_of_evaluate_split_maps_ensemble_significance_and_report(dev, world, tmp_path):
    from src.evaluation.metrics import evaluate_horizons
    from tecmollm import evaluate as E
    from tecmollm import significance as SG
    from tecmollm.ensemble import evaluate_ensemble
    model, ds, ei, scaler, lin = world["model"], world["test"], world["ei"], world["scaler"], world["lin"]
    with_l = E.evaluate_split(model, ds, ei, 64, scaler=scaler, baselines=("mean", "last", lin))
    without = E.evaluate_split(model, ds, ei, 64, scaler=scaler, baselines=("mean", "last"))
    assert list(with_l) == ["TEC-MoLLM", "HistoricalAverage", "Persistence", "Linear"]
    for name in without:
        _same(with_l[name], without[name], exact=True)
    pred = lin.forecast_windows(ds, range(len(ds)))
    assert pred.shape == (len(ds), L_OUT, 12, 1)
    _same(with_l["Linear"], evaluate_horizons(ds.batch(list(range(len(ds))))[2], pred, scaler), exact=False)
    assert with_l["Linear"]["rmse_avg"] < with_l["HistoricalAverage"]["rmse_avg"]
    assert with_l["Linear"]["rmse_avg"] < with_l["Persistence"]["rmse_avg"]
    res, maps = E.evaluate_maps(model, ds, ei, 64, scaler=scaler, baselines=("mean", lin))
    assert list(maps) == ["TEC-MoLLM", "HistoricalAverage", "Linear"] and maps["Linear"]["mae"].shape == (1, L_OUT, 12)
    _same(res["Linear"], with_l["Linear"], exact=True)
    imp = E.improvement(with_l, baseline="Linear")
    assert set(imp) == {"mae", "rmse", "r2_score", "pearson_r"} and all(np.isfinite(v) for v in imp.values())
    paths = E.write_report(with_l, str(tmp_path))
    assert "Linear:" in open(paths["summary"]).read() and "\nLinear," in open(paths["csv"]).read()
    eres, emaps, _ = evaluate_ensemble(model, ds, ei, 64, members=4, seed=3, scaler=scaler, trim=1, baselines=(lin,))
    assert list(eres) == ["TEC-MoLLM", "Linear", "TEC-MoLLM-MC"] and "Linear" in emaps
    _same(eres["Linear"], with_l["Linear"], exact=True)
    sres, sig = SG.evaluate_significance(model, ds, ei, 64, scaler=scaler, baselines=("mean", lin), replicates=40, seed=1)
    assert list(sres) == ["TEC-MoLLM", "HistoricalAverage", "Linear"] and "Linear" in sig["intervals"] and "Linear" in sig["dm"]
    _same(sres["Linear"], with_l["Linear"], exact=True)
    for bad in ("linear", 3, None):
        with pytest.raises(ValueError, match="baselines must come from"):
            E.evaluate_split(model, ds, ei, 64, scaler=scaler, baselines=("mean", bad))
    from src.models.baselines import LinearBaseline
    with pytest.raises(ValueError, match="must be fitted"):
        E.evaluate_split(model, ds, ei, 64, scaler=scaler, baselines=(LinearBaseline(device=dev),))


def test_round_trip_predict_and_the_two_dataset_kinds(dev, world, tmp_path):
    from src.data.dataset import SeriesWindowDataset, SlidingWindowSamplerDataset
    from src.models.baselines import LinearBaseline, load_baseline, save_baseline
    full, ds, lin, X, y, TF = world["full"], world["test"], world["lin"], world["X"], world["y"], world["TF"]
    save_baseline(lin, str(tmp_path / "linear.joblib"))
    back = load_baseline(str(tmp_path / "linear.joblib"))
    assert back._coef_dev is None and np.array_equal(back.coef_, lin.coef_) and np.array_equal(back.status_, lin.status_)
    idx = [0, 5, len(ds) - 1]
    assert torch.equal(back.forecast_windows(ds, idx), lin.forecast_windows(ds, idx))
    with pytest.raises(IndexError):
        lin.forecast_windows(ds, [len(ds)])
    # predict: the forecast from the end of the series the model was fitted on = the window that ends with X's last row
    last = (T_ALL - L_IN)                                   # its start; beyond the dataset's samples, so ask forecast_series
    want = lin.forecast_series(full.X.view(T_ALL, 12, 6), [last], L_IN, L_OUT).cpu().numpy()[0]
    out = lin.predict([3, 0, 11, 99], 5)
    assert sorted(out) == [0, 3, 11]
    for n, v in out.items():
        assert v.dtype == np.float64 and v.shape == (5,) and np.array_equal(v, want[:5, n].astype(np.float64))
    with pytest.raises(ValueError):
        lin.predict([0], L_OUT + 1)
    # the series dataset (reference windows) and the materialised dataset of the same data: the same windows, the same bits
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    ys = y.reshape(T_ALL, 3, 4)
    series = SeriesWindowDataset.from_series(t(X), t(ys), t(TF), L_IN, L_OUT, stride=2, device=dev, mode="train")
    Y = np.stack([ys[1 + h:T_ALL - L_OUT + 1 + h] for h in range(L_OUT)], axis=3)       # Y[i, :, :, h] = ys[i + 1 + h]
    mat = SlidingWindowSamplerDataset.from_tensors(t(X[:T_ALL - L_OUT]), t(Y), t(TF[:T_ALL - L_OUT]), L_IN, L_OUT, stride=2,
                                                   device=dev, mode="train")
    assert len(series) == len(mat) > 100
    for indices in (None, range(3, len(mat), 4)):
        a = LinearBaseline(lags=[1, 2, 12, 24], exog=[(3, 1)], alpha=0.5, device=dev).fit(series, indices)
        b = LinearBaseline(lags=[1, 2, 12, 24], exog=[(3, 1)], alpha=0.5, device=dev).fit(mat, indices)
        assert np.array_equal(a.coef_, b.coef_) and a.n_windows_ == b.n_windows_ and (a.status_ == 0).all()
    first, step, count = 3 * 2, 4 * 2, len(range(3, len(mat), 4))
    want, _, _ = LR.fit(X.reshape(T_ALL, 12, 6), y, a.pairs_, L_IN, L_OUT, first, step, count, 0.5)
    assert a.n_windows_ == count and np.abs(a.coef_ - want).max() <= 1e-9
    for bad in ([0, 1, 3], [5, 3, 1], []):
        with pytest.raises(ValueError):
            LinearBaseline(device=dev).fit(series, bad)
