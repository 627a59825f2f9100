"""GPU tests of the forecast combination: the moments (tecm_combine_moments), the per-cell solve (tecm_combine_solve) and the
blend (tecm_combine_apply) against the float64 numpy restatement of tests/combine_ref.py, and a fitted Combination inside
tecmollm.evaluate.

Bars.  Moments: the bits of the restatement on dyadic inputs (every product and sum is exact); on N(0, 1) inputs counts and
`skipped` exact and every sum within 1e-12 of the sum of its terms' magnitudes (the project's bar for ordered float64 sums).
Weights and intercept: 1e-9 absolute with cond(A) <= 1e4 asserted on the restatement, and the normal-equation residual
<= 1e-12 (|A| |w| + |b|) in the infinity norm with no condition cap (Cholesky is backward stable).  Blend: one float32 ulp of the
float64 restatement rounded to float32, both sides using the device's coefficients and member tensors."""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import combine_ref as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


LAYOUTS = ("permuted", "contiguous", "broadcast", "strided")


def place(dev, a, layout):
    """(S, H, I) float32 numpy -> ((S, H, I) device view in `layout`, the values it holds).  "permuted": the model's storage
    (S, I, H) seen as (S, H, I), stride_h = 1 and stride_i = H; "broadcast": one value per (sample, node), stride_h = 0 (the
    values of horizon 0); "strided": every other node of every other sample of a wider tensor."""
    t = torch.tensor(a)
    if layout == "permuted":
        return t.permute(0, 2, 1).contiguous().to(dev).permute(0, 2, 1), a
    if layout == "broadcast":
        return t[:, :1].contiguous().to(dev).expand(a.shape), np.broadcast_to(a[:, :1], a.shape)
    if layout == "strided":
        wide = torch.full((2 * a.shape[0], a.shape[1], 2 * a.shape[2] + 1), float("nan"))
        wide[::2, :, 1::2] = t
        return wide.to(dev)[::2, :, 1::2], a
    return t.to(dev), a


def operands(dev, rng, S, H, I, M, rotate, values):
    """M members and a target in rotating layouts.  values "dyadic": multiples of 1/4 in [-4, 4]; "normal": N(0, 1) with NaN
    and +-inf sprinkled into every operand."""
    arrays = []
    for o in range(M + 1):
        if values == "dyadic":
            a = (rng.integers(-16, 17, (S, H, I)) / 4.0).astype(np.float32)
        else:
            a = rng.standard_normal((S, H, I)).astype(np.float32)
            flat = a.reshape(-1)
            hit = rng.integers(0, flat.size, max(1, flat.size // 40))
            flat[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), hit.size)
        arrays.append(a)
    placed = [place(dev, a, LAYOUTS[(rotate + o) % 4]) for o, a in enumerate(arrays[:M])]
    target = place(dev, arrays[M], ("contiguous", "permuted", "strided")[rotate % 3])
    return [p[0] for p in placed], [p[1] for p in placed], target[0], target[1]


def group_ids(dev, rng, S, G):
    """G = 3: ids from {0, 2} only -- group 1 never occurs."""
    if G == 1:
        return None, None
    ids = rng.choice(np.array([0, 2], dtype=np.int32), S)
    return torch.tensor(ids).to(dev), ids


def check_moments(got, want, scale, M, what):
    K = CR.moment_count(M)
    assert np.array_equal(got[:, :, 0], want[:, :, 0]) and np.array_equal(got[:, :, K - 1], want[:, :, K - 1]), what
    err = np.abs(got - want)
    assert (err <= 1e-12 * scale).all(), (what, float((err / np.maximum(scale, 1e-300)).max()))


# ------------------------------------------------------------------------------------ moments
SENTINEL = 7.5


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 8])
def test_moments_every_shape_layout_and_bucket(dev, M):
    """I in {1, 63, 64, 65, 135} x H in {1, 12, 50}, with S in {1, 5, 17} (17 crosses every bucket's samples in flight: 16, 16,
    8, 4), G in {1, 3} and the layouts rotating over the fifteen shapes; H = 12 takes the LDS route for the permuted operands,
    H = 50 and H = 1 read them in place.  Statistics pre-filled with a sentinel: the group that never occurs keeps it."""
    from tecmollm.combine import CombinationMoments
    rng = np.random.default_rng(100 + M)
    for c, (I, H) in enumerate(itertools.product((1, 63, 64, 65, 135), (1, 12, 50))):
        S, G = (1, 5, 17)[(c + M) % 3], (1, 3)[(c // 3 + M) % 2]
        for values in ("dyadic", "normal"):
            preds, pred_values, y, y_values = operands(dev, rng, S, H, I, M, c + M, values)
            ids, ids_host = group_ids(dev, rng, S, G)
            cm = CombinationMoments([f"m{m}" for m in range(M)], H, I, G, device=dev)
            cm.stats.fill_(SENTINEL)
            cm.update(preds, y, ids)
            got = cm.stats.cpu().numpy()
            base = np.full(got.shape, SENTINEL)
            want = CR.moments(pred_values, y_values, ids_host, G, stats=base)
            what = (M, I, H, S, G, values)
            if G == 3:
                assert (got[1] == SENTINEL).all(), what
            if values == "dyadic":
                assert np.array_equal(got, want), what
            else:
                scale = CR.moments(pred_values, y_values, ids_host, G, stats=base, absolute=True)
                check_moments(got, want, scale, M, what)
    torch.cuda.synchronize()


def test_moments_the_route_does_not_change_a_bit(dev):
    """The same values as the permuted view (LDS route at H = 12) and as contiguous tensors (read in place): equal bits."""
    from tecmollm.combine import CombinationMoments
    rng = np.random.default_rng(7)
    for M, H in ((2, 12), (4, 12), (8, 32), (3, 33)):
        arrays = [rng.standard_normal((9, H, 70)).astype(np.float32) for _ in range(M + 1)]
        stats = []
        for layout in ("permuted", "contiguous"):
            cm = CombinationMoments([f"m{m}" for m in range(M)], H, 70, device=dev)
            ops = [place(dev, a, layout)[0] for a in arrays]
            cm.update(ops[:M], ops[M])
            stats.append(cm.stats.clone())
        assert torch.equal(stats[0], stats[1]), (M, H)


def test_moments_accumulate_are_reproducible_and_report_a_bad_group(dev):
    from tecmollm import check_device_errors
    from tecmollm._lib import TecmError
    from tecmollm.combine import CombinationMoments
    rng = np.random.default_rng(11)
    S, H, I, M, G = 23, 12, 65, 3, 3
    preds, pred_values, y, y_values = operands(dev, rng, S, H, I, M, 0, "normal")
    ids_host = rng.integers(0, G, S).astype(np.int32)
    ids = torch.tensor(ids_host).to(dev)
    names = ["a", "b", "c"]
    one = CombinationMoments(names, H, I, G, device=dev)
    one.update(dict(zip(names, preds)), y, ids)
    runs = []
    for _ in range(2):
        again = CombinationMoments(names, H, I, G, device=dev)
        again.update(preds, y, ids)
        runs.append(again.stats)
    assert torch.equal(runs[0], one.stats) and torch.equal(runs[1], one.stats)
    two = CombinationMoments(names, H, I, G, device=dev)
    two.update([p[:10] for p in preds], y[:10], ids[:10])
    two.update([p[10:] for p in preds], y[10:], ids[10:])
    scale = CR.moments(pred_values, y_values, ids_host, G, absolute=True)
    check_moments(two.stats.cpu().numpy(), one.stats.cpu().numpy(), scale, M, "two updates")
    check_moments(one.stats.cpu().numpy(), CR.moments(pred_values, y_values, ids_host, G), scale, M, "one update")
    check_device_errors(dev)
    # a bad id: the sample is skipped, never clamped, and the device error word reports it
    bad_host = ids_host.copy()
    bad_host[[3, 17]] = (G, -1)
    bad = CombinationMoments(names, H, I, G, device=dev)
    bad.update(preds, y, torch.tensor(bad_host).to(dev))
    check_moments(bad.stats.cpu().numpy(), CR.moments(pred_values, y_values, bad_host, G), scale, M, "bad ids")
    assert bad.stats[:, :, 0].sum().item() + bad.stats[:, :, -1].sum().item() == (S - 2) * H * I
    with pytest.raises(TecmError, match="TECM_BAD_GROUP"):
        check_device_errors(dev)
    check_device_errors(dev)                                               # the word is cleared once reported
    with pytest.raises(ValueError, match="groups"):
        bad.update(preds, y, None)
    with pytest.raises(ValueError, match="shape mismatch"):
        bad.update([p[:, :6] for p in preds], y[:, :6], ids)


# ------------------------------------------------------------------------------------ solve
def norm_inf(a):
    return np.abs(a).sum(axis=-1).max(axis=-1)


def device_fit(dev, stats, names, H, I, G=1, **kw):
    from tecmollm.combine import CombinationMoments
    cm = CombinationMoments(names, H, I, G, device=dev)
    cm.stats.copy_(torch.from_numpy(np.ascontiguousarray(stats)))
    return cm, cm.fit(**kw)


def residual_check(stats, weight, ridge, w0, what):
    """|A w - b| <= 1e-12 (|A| |w| + |b|) over the kept members of every solved cell."""
    M, n, _, _, A, b = CR.system(np.moveaxis(stats, 2, -1), ridge, w0)
    w = np.moveaxis(weight, 2, -1)                                          # (G, H, I, M)
    keep = (w != 0)[..., None, :] & (w != 0)[..., :, None]
    Ak = np.where(keep, A, 0.0)
    res = np.abs(np.einsum("...mk,...k->...m", Ak, w) - np.where(w != 0, b, 0.0)).max(axis=-1)
    bound = 1e-12 * (norm_inf(Ak) * np.abs(w).max(axis=-1) + np.abs(b).max(axis=-1))
    assert (res <= bound).all(), (what, float((res / bound).max()))


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("ridge", [0.0, 0.01])
def test_solve_matches_the_restatement_and_the_normal_equations(dev, M, ridge):
    H, I = 3, 70
    preds, y = CR.members_and_truth(20 + M, 80, H, I, M)
    stats = CR.moments(preds, y)
    names = [f"m{m}" for m in range(M)]
    prior = None if M != 3 else [0.5, 0.25, 0.25]
    _, comb = device_fit(dev, stats, names, H, I, ridge=ridge, prior=prior)
    w0 = np.full(M, 1.0 / M) if prior is None else np.asarray(prior)
    weight, intercept, status, dropped, cond = CR.solve(stats, ridge, w0)
    assert comb.weight.shape == (1, H, M, I) and comb.weight.dtype == np.float64 and comb.status.dtype == np.int32
    assert comb.dropped.dtype == np.uint8 and not comb.status.any() and not status.any() and not comb.dropped.any()
    assert cond.max() <= 1e4, cond.max()
    assert np.abs(comb.weight - weight).max() <= 1e-9 and np.abs(comb.intercept - intercept).max() <= 1e-9
    assert np.array_equal(comb.counts, stats[:, :, 0]) and not comb.skipped.any()
    residual_check(stats, comb.weight, ridge, w0, (M, ridge))
    assert (comb.ridge, comb.pool, comb.member_names) == (ridge, "cell", names)


def test_solve_duplicates_and_the_fallbacks(dev):
    """Member 2 is a copy of member 0 (dropped at ridge 0, an equal share at ridge 0.01), member 3 of one node is constant;
    group 1 holds one sample (FEW), group 2 none (EMPTY), one cell holds an infinite moment (NONFINITE)."""
    H, I, G = 2, 66, 3
    preds, y = CR.members_and_truth(31, 60, H, I, 3)
    preds = [preds[0], preds[1], preds[0].copy(), preds[2].copy()]
    preds[3][:, :, 5] = 3.25
    ids = np.zeros(60, dtype=np.int32)
    ids[59] = 1
    stats = CR.moments(preds, y, ids, G)
    stats[0, 1, 4, 64] = np.inf
    names = ["a", "b", "twin", "c"]
    w0 = np.array([0.3, 0.4, 0.3, 0.1])                                    # the twins share their prior, so they share their weight
    for ridge in (0.0, 0.01):
        _, comb = device_fit(dev, stats, names, H, I, G, ridge=ridge, prior=w0)
        weight, intercept, status, dropped, _ = CR.solve(stats, ridge, w0)
        assert np.array_equal(comb.status, status) and np.array_equal(comb.dropped, dropped), ridge
        assert np.abs(comb.weight - weight).max() <= 1e-9 and np.abs(comb.intercept - intercept).max() <= 1e-9
        assert (comb.status[2] == CR.EMPTY).all() and (comb.status[1] == CR.FEW).all() and comb.status[0, 1, 64] == CR.NONFINITE
        for cell in ((2, 0, 0), (1, 1, 3), (0, 1, 64)):
            assert comb.weight[cell[0], cell[1], :, cell[2]].tolist() == w0.tolist()
        assert (comb.intercept[2] == 0).all() and comb.intercept[0, 1, 64] == 0 and (comb.intercept[1] != 0).all()
        solved = (comb.status[0] & (CR.FEW | CR.EMPTY | CR.NONFINITE)) == 0                 # (H, I)
        if ridge == 0.0:
            assert ((comb.dropped[0][solved] & 0b100) != 0).all() and (comb.weight[0, :, 2][solved] == 0).all()
            assert comb.dropped[0, 0, 5] == 0b1100 and comb.status[0, 0, 5] == CR.DROPPED
            plain = CR.solve(CR.moments([preds[0], preds[1], preds[3]], y, ids, G), 0.0, w0[[0, 1, 3]])[0]
            assert np.abs(comb.weight[0][:, [0, 1, 3]].transpose(0, 2, 1)[solved] - plain[0].transpose(0, 2, 1)[solved]).max() <= 1e-9
        else:
            assert not (comb.dropped[0][solved] & 0b0111).any()
            assert np.abs(comb.weight[0, :, 0] - comb.weight[0, :, 2])[solved].max() <= 1e-9
        keep = np.broadcast_to((comb.status == 0) | (comb.status == CR.DROPPED), comb.status.shape)
        st = np.where(keep[:, :, None, :], stats, CR.moments(preds, y)[0:1])        # fallback cells: any solvable system
        residual_check(st, np.where(keep[:, :, None, :], comb.weight, 0.0), ridge, w0, ("fallbacks", ridge))


@pytest.mark.parametrize("pool", ["horizon", "all"])
def test_pooled_fits_equal_the_fit_of_the_summed_moments(dev, pool):
    H, I, M, G = 3, 70, 4, 2
    preds, y = CR.members_and_truth(41, 50, H, I, M)
    ids = (np.arange(50) % 2).astype(np.int32)
    stats = CR.moments(preds, y, ids, G)
    cm, comb = device_fit(dev, stats, [f"m{m}" for m in range(M)], H, I, G, pool=pool)
    pooled = cm.pooled_stats(pool).cpu().numpy()
    summed = stats.sum(axis=3, keepdims=True) if pool == "horizon" else stats.sum(axis=(1, 3), keepdims=True)
    assert pooled.shape == summed.shape and (np.abs(pooled - summed) <= 1e-12 * np.abs(stats).sum(axis=(1, 3), keepdims=True)).all()
    weight, intercept, status, dropped, cond = CR.solve(pooled)
    assert cond.max() <= 1e4 and not status.any()
    assert comb.weight.shape == (G, H, M, I) and comb.weight.strides[3] == 0 and comb.intercept.strides[2] == 0
    assert (comb.weight.strides[1] == 0) == (pool == "all") and comb.pool == pool
    assert np.abs(comb.weight - weight).max() <= 1e-9 and np.abs(comb.intercept - intercept).max() <= 1e-9
    assert np.array_equal(comb.counts, np.broadcast_to(pooled[:, :, 0], (G, H, I)))


# ------------------------------------------------------------------------------------ apply
def ulp_check(got, want64, what):
    want = want64.astype(np.float32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    assert np.isfinite(got).all() and (err <= ulp).all(), (what, float((err / ulp).max()))


@pytest.mark.parametrize("H", [1, 12, 13])
def test_apply_matches_the_restatement_within_one_ulp(dev, H):
    """B = 1 and 5, N = 135, three members in rotating layouts, per-cell and pooled (stride-0) coefficients, G = 1 and 3; the
    output plain, strided and permuted."""
    from tecmollm.combine import Combination
    rng = np.random.default_rng(50 + H)
    N, M = 135, 3
    names = ["a", "b", "c"]
    for pool, G in (("cell", 1), ("horizon", 1), ("all", 3), ("cell", 3)):
        Hs, Ns = (H, N) if pool == "cell" else ((H, 1) if pool == "horizon" else (1, 1))
        zeros = np.zeros((G, Hs, Ns))
        comb = Combination(rng.standard_normal((G, Hs, M, Ns)), rng.standard_normal((G, Hs, Ns)), zeros, zeros, zeros, zeros,
                           names, (H, N), pool=pool)
        for B in (1, 5):
            placed = [place(dev, rng.standard_normal((B, H, N)).astype(np.float32), LAYOUTS[(m + B) % 4]) for m in range(M)]
            ids_host = rng.integers(0, G, B).astype(np.int32) if G > 1 else None
            ids = None if ids_host is None else torch.tensor(ids_host).to(dev)
            want = CR.apply(comb.weight, comb.intercept, [p[1] for p in placed], ids_host)
            preds = dict(zip(names, (p[0] for p in placed)))
            plain = comb.combine(preds, ids)
            assert plain.shape == (B, H, N, 1) and plain.dtype == torch.float32
            ulp_check(plain[..., 0].cpu().numpy(), want, (H, pool, G, B))
            wide = torch.full((B, H, 2 * N), -7.0, device=dev)
            comb.combine(preds, ids, out=wide[:, :, ::2])
            perm = torch.empty(N, B, H, device=dev)
            comb.combine(preds, ids, out=perm.permute(1, 2, 0))
            assert torch.equal(wide[:, :, ::2], plain[..., 0]) and (wide[:, :, 1::2] == -7.0).all()
            assert torch.equal(perm.permute(1, 2, 0), plain[..., 0])
            assert torch.equal(comb.combine({k: v.unsqueeze(-1) for k, v in preds.items()}, ids), plain)


def test_apply_propagates_non_finite_members_and_marks_a_bad_group(dev):
    from tecmollm import check_device_errors
    from tecmollm._lib import TecmError
    from tecmollm.combine import Combination
    rng = np.random.default_rng(61)
    B, H, N, G = 4, 12, 65, 3
    zeros = np.zeros((G, H, N))
    comb = Combination(rng.standard_normal((G, H, 2, N)), rng.standard_normal((G, H, N)), zeros, zeros, zeros, zeros, ["a", "b"], (H, N))
    a, b = (rng.standard_normal((B, H, N)).astype(np.float32) for _ in range(2))
    a[1, 3, 7], b[2, 0, 64] = np.nan, np.inf
    preds = {"a": torch.tensor(a).to(dev), "b": torch.tensor(b).to(dev)}
    ids_host = np.array([0, 2, 1, 2], dtype=np.int32)
    out = comb.combine(preds, torch.tensor(ids_host).to(dev))[..., 0].cpu().numpy()
    want = CR.apply(comb.weight, comb.intercept, [a, b], ids_host)
    assert np.isnan(out[1, 3, 7]) and not np.isfinite(out[2, 0, 64]) and np.isfinite(out).sum() == out.size - 2
    clean = np.isfinite(want)
    ulp_check(out[clean], want[clean], "non-finite members")
    check_device_errors(dev)
    ids_host[1] = 3
    out = comb.combine(preds, torch.tensor(ids_host).to(dev))[..., 0].cpu().numpy()
    assert np.isnan(out[1]).all() and np.isfinite(out[[0, 3]]).all()
    with pytest.raises(TecmError, match="TECM_BAD_GROUP"):
        check_device_errors(dev)
    with pytest.raises(ValueError, match="groups"):
        comb.combine(preds)
    with pytest.raises(ValueError, match="missing"):
        comb.combine({"a": preds["a"]})


# ------------------------------------------------------------------------------------ end to end
KEYS = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg", "mae_by_horizon", "rmse_by_horizon", "r2_by_horizon",
        "pearson_by_horizon")
L_IN, L_OUT, T_ALL = 48, 12, 600
KINDS = ("mean", "last", "periodic")


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.fixture(scope="module")
def world(dev):
    """A 12-node model and a split of its own: 600 steps of the seasonal generator (seed 1) as channel 0 of X and as the
    target series.  `fit` holds the first two thirds of the stride-1 windows, `test` the last third."""
    from oracle import ref_cpu as R
    from src.data.dataset import SeriesWindowDataset
    from tests.parity import build_model
    rng = np.random.default_rng(21)
    y = CR.world_series()
    X = rng.standard_normal((T_ALL, 3, 4, 6)).astype(np.float32)
    X[:, :, :, 0] = y.reshape(T_ALL, 3, 4)
    TF = np.stack([rng.integers(0, 12, T_ALL), rng.integers(0, 366, T_ALL), rng.integers(0, 13, T_ALL),
                   rng.integers(0, 4, T_ALL)], axis=1).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    S = T_ALL - L_IN - L_OUT + 1
    n_fit = 2 * S // 3
    rows = n_fit + L_IN + L_OUT - 1
    make = lambda lo, hi: SeriesWindowDataset.from_series(t(X[lo:hi]), t(y[lo:hi].reshape(-1, 3, 4)), t(TF[lo:hi]), L_IN, L_OUT,
                                                          device=dev, mode="test", windows="all")
    fit, test = make(0, rows), make(n_fit, T_ALL)
    assert len(fit) == n_fit and len(test) == S - n_fit
    cfg = R.default_config(L_in=L_IN, L_out=L_OUT, num_nodes=12)
    model = build_model(cfg, R.init_params(cfg, seed=3), dev, "per_timestep").eval()
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev)
    return dict(y=y, fit=fit, test=test, n_fit=n_fit, model=model, ei=ei, scaler=(20.0, 7.0))


def members_of(ds, kinds=KINDS):
    from tecmollm import evaluate as E
    idx = list(range(len(ds)))
    return {k: E.window_baseline(ds, idx, k) for k in kinds}, ds.batch(idx)[2]


def host(t):
    return t[..., 0].cpu().numpy()


@pytest.fixture(scope="module")
def fitted(dev, world):
    from tecmollm.combine import fit_combination
    return {ridge: fit_combination(world["model"], world["fit"], world["ei"], 64, members=KINDS, ridge=ridge)
            for ridge in (0.0, 0.01)}


def test_the_window_baselines_blend_beats_every_member_on_held_out_windows(dev, world, fitted):
    want_rmse = {0.0: 1.118, 0.01: 1.108, "mean": 1.208, "periodic": 1.363, "last": 1.627}
    ref = {ridge: CR.held_out(world["y"], ridge=ridge) for ridge in (0.0, 0.01)}
    test_members, truth = members_of(world["test"])
    fit_members, fit_truth = members_of(world["fit"])
    for ridge, comb in fitted.items():
        assert comb.weight.shape == (1, L_OUT, 3, 12) and comb.member_names == list(KINDS) and comb.name == "Combination"
        assert (comb.counts == world["n_fit"]).all() and not comb.skipped.any()
        # the fit is the restatement's on the device's own member tensors
        stats = CR.moments([host(fit_members[k]) for k in KINDS], host(fit_truth))
        weight, intercept, status, dropped, cond = CR.solve(stats, ridge)
        assert np.array_equal(comb.status, status) and np.array_equal(comb.dropped, dropped)
        ok = cond <= 1e4
        assert ok.sum() >= 100 and np.abs(comb.weight - weight).transpose(0, 1, 3, 2)[ok].max() <= 1e-9
        assert np.abs(comb.intercept - intercept)[ok].max() <= 1e-9
        # the dropped pattern: "periodic" is "last" at horizon index 11, and only there
        if ridge == 0.0:
            assert (comb.dropped[0, 11] == 0b100).all() and not comb.dropped[0, :11].any()
            assert (comb.status[0, 11] == CR.DROPPED).all() and (comb.weight[0, 11, 2] == 0).all()
        else:
            assert not comb.dropped.any() and not comb.status.any()
        assert np.array_equal(comb.dropped, ref[ridge]["dropped"])
        # held out: one float32 ulp of the restatement on the device's members, and better than every member
        idx = list(range(len(world["test"])))
        x, tf, _ = world["test"].batch(idx)
        blend = comb.forecast(world["model"], x, tf, world["ei"], world["test"], idx)
        assert blend.shape == (len(idx), L_OUT, 12, 1)
        ulp_check(host(blend), CR.apply(comb.weight, comb.intercept, [host(test_members[k]) for k in KINDS]), ridge)
        rmse = {k: CR.rmse(host(test_members[k]), host(truth)) for k in KINDS}
        rmse[ridge] = CR.rmse(host(blend), host(truth))
        print(ridge, rmse)
        assert all(rmse[ridge] < rmse[k] for k in KINDS)
        for k in (ridge,) + KINDS:
            assert abs(rmse[k] - want_rmse[k]) <= 5e-4, (k, rmse[k])
    # in-sample at ridge 0, per cell: least squares is never beaten by a unit vector, up to the blend's float32 rounding
    blend = host(fitted[0.0].combine(fit_members)).astype(np.float64)
    res = host(fit_truth).astype(np.float64) - blend
    slack = 2.0 ** -23 * (np.abs(res) * np.abs(blend)).sum(axis=0)
    for k in KINDS:
        member_sse = ((host(fit_truth).astype(np.float64) - host(fit_members[k]).astype(np.float64)) ** 2).sum(axis=0)
        assert ((res ** 2).sum(axis=0) <= member_sse + slack).all(), k


def test_one_member_is_the_affine_recalibration_of_the_model(dev, world):
    from tecmollm.combine import fit_combination
    from tecmollm.loop import _batches
    model, ds, ei = world["model"], world["fit"], world["ei"]
    comb = fit_combination(model, ds, ei, 64, members=("model",))
    outs, truths = [], []
    with torch.no_grad():
        for chunk in _batches(len(ds), 64):
            x, tf, y = ds.batch(chunk)
            outs.append(host(model(x, tf, ei)))
            truths.append(host(y))
    p, t = np.concatenate(outs).astype(np.float64), np.concatenate(truths).astype(np.float64)
    assert comb.weight.shape == (1, L_OUT, 1, 12) and comb.member_names == ["model"] and not comb.status.any()
    pc, tc = p - p.mean(axis=0), t - t.mean(axis=0)
    slope = (pc * tc).sum(axis=0) / (pc * pc).sum(axis=0)
    assert np.abs(comb.weight[0, :, 0] - slope).max() <= 1e-6 * np.abs(slope).max()       # the centred textbook formula
    assert np.abs(comb.intercept[0] - (t.mean(axis=0) - slope * p.mean(axis=0))).max() <= 1e-6
    weight, intercept, _, _, _ = CR.solve(CR.moments([p.astype(np.float32)], t.astype(np.float32)))
    assert np.abs(comb.weight - weight).max() <= 1e-9 and np.abs(comb.intercept - intercept).max() <= 1e-9
    idx = [0, 5, 17]
    x, tf, _ = ds.batch(idx)
    blend = comb.forecast(model, x, tf, ei, ds, idx)
    with torch.no_grad():
        out = host(model(x, tf, ei))
    ulp_check(host(blend), CR.apply(comb.weight, comb.intercept, [out]), "recalibration")


def test_a_combination_is_a_baseline_of_evaluate_split_maps_ensemble_significance_and_report(dev, world, fitted, tmp_path):
    from src.evaluation.metrics import evaluate_horizons
    from tecmollm import evaluate as E
    from tecmollm import significance as SG
    from tecmollm.combine import Combination, fit_combination, write_combination
    from tecmollm.ensemble import evaluate_ensemble
    model, ds, ei, scaler, comb = world["model"], world["test"], world["ei"], world["scaler"], fitted[0.01]
    with_c = E.evaluate_split(model, ds, ei, 64, scaler=scaler, baselines=("mean", comb, "last"))
    without = E.evaluate_split(model, ds, ei, 64, scaler=scaler, baselines=("mean", "last"))
    assert list(with_c) == ["TEC-MoLLM", "HistoricalAverage", "Combination", "Persistence"]
    for name in without:
        _same(with_c[name], without[name])
    idx = list(range(len(ds)))
    x, tf, truth = ds.batch(idx)
    want = evaluate_horizons(truth, comb.forecast(model, x, tf, ei, ds, idx), scaler)
    for k in KEYS:
        np.testing.assert_allclose(np.asarray(with_c["Combination"][k]), np.asarray(want[k]), rtol=1e-12, atol=0, err_msg=k)
    assert with_c["Combination"]["rmse_avg"] < min(with_c["HistoricalAverage"]["rmse_avg"], with_c["Persistence"]["rmse_avg"])
    imp = E.improvement(with_c, baseline="Combination")
    assert set(imp) == {"mae", "rmse", "r2_score", "pearson_r"} and all(np.isfinite(v) for v in imp.values())
    paths = E.write_report(with_c, str(tmp_path))
    assert "Combination:" in open(paths["summary"]).read() and "\nCombination," in open(paths["csv"]).read()
    # a member that is not listed is computed for the combination alone; the entry does not depend on what else is listed
    alone = E.evaluate_split(model, ds, ei, 64, scaler=scaler, baselines=(comb,))
    assert list(alone) == ["TEC-MoLLM", "Combination"]
    _same(alone["Combination"], with_c["Combination"])
    # with the model as a member, under another name
    stacked = fit_combination(model, world["fit"], ei, 64, members=("model", "mean", "periodic"), ridge=0.01, name="Stack")
    both = E.evaluate_split(model, ds, ei, 64, scaler=scaler, baselines=(stacked, "mean", comb))
    assert list(both) == ["TEC-MoLLM", "Stack", "HistoricalAverage", "Combination"]
    _same(both["Combination"], with_c["Combination"])
    _same(both["TEC-MoLLM"], without["TEC-MoLLM"])
    assert both["Stack"]["rmse_avg"] < both["TEC-MoLLM"]["rmse_avg"]
    res, maps = E.evaluate_maps(model, ds, ei, 64, scaler=scaler, baselines=("mean", comb))
    assert list(maps) == ["TEC-MoLLM", "HistoricalAverage", "Combination"] and maps["Combination"]["mae"].shape == (1, L_OUT, 12)
    _same(res["Combination"], with_c["Combination"])
    _same(res["HistoricalAverage"], without["HistoricalAverage"])
    eres, emaps, _ = evaluate_ensemble(model, ds, ei, 64, members=4, seed=3, scaler=scaler, trim=1, baselines=(comb,))
    eplain, _, _ = evaluate_ensemble(model, ds, ei, 64, members=4, seed=3, scaler=scaler, trim=1, baselines=())
    assert list(eres) == ["TEC-MoLLM", "Combination", "TEC-MoLLM-MC"] and "Combination" in emaps
    _same(eres["Combination"], with_c["Combination"])
    for name in eplain:
        _same(eres[name], eplain[name])
    sres, sig = SG.evaluate_significance(model, ds, ei, 64, scaler=scaler, baselines=("mean", comb), replicates=40, seed=1)
    splain, _ = SG.evaluate_significance(model, ds, ei, 64, scaler=scaler, baselines=("mean",), replicates=40, seed=1)
    assert list(sres) == ["TEC-MoLLM", "HistoricalAverage", "Combination"]
    assert "Combination" in sig["intervals"] and "Combination" in sig["dm"]
    _same(sres["Combination"], with_c["Combination"])
    for name in splain:
        _same(sres[name], splain[name])
    with pytest.raises(ValueError, match="collides"):
        E.evaluate_split(model, ds, ei, 64, scaler=scaler, baselines=(comb, fitted[0.0]))
    # files: save / load gives the same forecast; the maps and the table are written
    back = Combination.load(comb.save(str(tmp_path / "comb.npz")))
    assert torch.equal(back.forecast(model, x[:5], tf[:5], ei, ds, idx[:5]), comb.forecast(model, x[:5], tf[:5], ei, ds, idx[:5]))
    out = write_combination(comb, str(tmp_path), grid=(3, 4))
    with np.load(out["npz"]) as z:
        assert z["weight"].shape == (1, L_OUT, 3, 3, 4) and z["status"].shape == (1, L_OUT, 3, 4)
    assert len(open(out["csv"]).read().splitlines()) == 1 + L_OUT


def test_a_grouped_combination_needs_the_evaluations_groups(dev, world):
    from tecmollm import evaluate as E
    from tecmollm.combine import fit_combination
    model, ei, scaler = world["model"], world["ei"], world["scaler"]
    fit_groups = (torch.arange(len(world["fit"]), device=dev) % 3).to(torch.int32)
    test_groups = (torch.arange(len(world["test"]), device=dev) % 3).to(torch.int32)
    comb = fit_combination(model, world["fit"], ei, 64, members=("mean", "periodic"), groups=fit_groups, num_groups=3, ridge=0.01)
    assert comb.G == 3 and comb.weight.shape == (3, L_OUT, 2, 12) and not comb.status.any()
    per_group = [len(range(g, len(world["fit"]), 3)) for g in range(3)]
    assert [int(comb.counts[g, 0, 0]) for g in range(3)] == per_group
    members, truth = members_of(world["fit"], ("mean", "periodic"))
    want = CR.solve(CR.moments([host(members[k]) for k in ("mean", "periodic")], host(truth), fit_groups.cpu().numpy(), 3), 0.01)
    assert np.abs(comb.weight - want[0]).max() <= 1e-9 and np.abs(comb.intercept - want[1]).max() <= 1e-9
    res, maps = E.evaluate_maps(model, world["test"], ei, 64, scaler=scaler, baselines=("mean", comb), groups=test_groups, num_groups=3)
    assert list(res) == ["TEC-MoLLM", "HistoricalAverage", "Combination"] and maps["Combination"]["rmse"].shape == (3, L_OUT, 12)
    assert res["Combination"]["rmse_avg"] < res["HistoricalAverage"]["rmse_avg"]
    with pytest.raises(ValueError, match="fitted with 3 groups"):
        E.evaluate_split(model, world["test"], ei, 64, scaler=scaler, baselines=("mean", comb))
    with pytest.raises(ValueError, match="fitted with 3 groups"):
        E.evaluate_maps(model, world["test"], ei, 64, scaler=scaler, baselines=(comb,), groups=test_groups, num_groups=4)
    with pytest.raises(ValueError, match="groups"):
        fit_combination(model, world["fit"], ei, 64, members=("mean",), num_groups=3)
    for bad, text in ((("mean", "mean"), "unique"), (("model",) * 9, "1 to 8"), (("median",), "a member is")):
        with pytest.raises(ValueError, match=text):
            fit_combination(model, world["fit"], ei, 64, members=bad)


# ------------------------------------------------------------------------------------ ranks
def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_sums(rank):
    g = torch.Generator().manual_seed(70 + rank)
    return torch.rand((2, 3, CR.moment_count(3), 6), generator=g, dtype=torch.float64) * 100


def _merge_worker(rank, port, out_dir):
    import sys
    import torch.distributed as dist
    for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from tecmollm.combine import CombinationMoments
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    try:
        cm = CombinationMoments(["a", "b", "c"], 3, 6, 2, device="cpu")
        cm.stats.copy_(_rank_sums(rank))
        assert cm.merge_() is cm
        torch.save({"stats": cm.stats}, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_merge_on_two_gloo_ranks_is_the_plain_sum(tmp_path):
    """The moments of two ranks (host tensors: the ranks open no GPU) after `merge_`: the plain sum, on both ranks."""
    import torch.multiprocessing as mp
    mp.spawn(_merge_worker, args=(_free_port(), str(tmp_path)), nprocs=2, join=True)
    s0, s1 = _rank_sums(0), _rank_sums(1)
    for rank in (0, 1):
        got = torch.load(os.path.join(tmp_path, f"rank{rank}.pt"))
        assert torch.equal(got["stats"], s0 + s1)
