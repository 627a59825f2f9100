"""GPU tests of the conformal intervals: the exact selection (tecm_column_select) against `np.sort`, the scores
(tecm_conformal_scores) bit for bit and the interval statistics (tecm_interval_stats) against the ordered float64 restatement
(tests/conformal_ref.py), the exact self-consistency of calibrating and scoring one split, the coverage theory promises on
exchangeable synthetic scores, and calibrate / evaluate / forecast / write end to end on a tiny model.

Bars: the selection, the scores and the four counts are exact.  The two sums (width, Winkler) are held to the error maps'
bar (tests/test_gpu_error_maps.py): |kernel - numpy| <= 1e-12 * sum |terms|, both sides adding the same float64 terms in the
same order, so only FMA contraction inside a term lies between them."""
import os

import numpy as np
import pytest
import torch

from tests import conformal_ref as CR

pytestmark = pytest.mark.gpu

BAR = 1e-12
SCALER = (21.5, 9.25)
KINDS = 9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


# ------------------------------------------------------------------------------------ selection
def _column(kind, S, rng):
    """One column of S float32 values of one of the KINDS value sets."""
    u32 = lambda a: np.asarray(a, dtype=np.uint32).view(np.float32)
    if kind == 0:                                                          # continuous
        return rng.standard_normal(S).astype(np.float32) * 3
    if kind == 1:                                                          # quantised to 0.25: heavy ties, both zeros
        v = (np.round(rng.standard_normal(S) * 2) / 4).astype(np.float32)
        v[(v == 0) & (rng.random(S) < 0.5)] = np.float32(-0.0)
        return v
    if kind == 2:                                                          # constant
        return np.full(S, 7.5, dtype=np.float32)
    if kind == 3:                                                          # both infinities among ordinary values
        v = rng.standard_normal(S).astype(np.float32)
        v[rng.random(S) < 0.2] = np.inf
        v[rng.random(S) < 0.2] = -np.inf
        return v
    if kind == 4:                                                          # NaN of both signs, quiet and with payloads
        v = rng.standard_normal(S).astype(np.float32)
        nan = u32(rng.choice(np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff812345, 0x7fffffff], dtype=np.uint32), S))
        return np.where(rng.random(S) < 0.3, nan, v)
    if kind == 5:                                                          # denormals of both signs
        return u32(rng.integers(1, 1 << 23, S).astype(np.uint32) | (rng.integers(0, 2, S).astype(np.uint32) << 31))
    if kind == 6:                                                          # negatives only
        return -np.abs(rng.standard_normal(S).astype(np.float32)) - np.float32(0.5)
    if kind == 7:                                                          # only the lowest byte differs: the last pass decides
        return u32(np.uint32(0x40490f00) | rng.integers(0, 256, S).astype(np.uint32))
    return u32((rng.integers(0, 256, S).astype(np.uint32) << 24) | np.uint32(0x00490fdb))   # only the top byte: the first pass


def _matrix(S, C, rng, first_kind=0):
    return np.stack([_column((first_kind + c) % KINDS, S, rng) for c in range(C)], axis=1)


def _group_ids(S, G):
    """One group: all zeros.  Three: group 1 is empty and group 2 holds the last row alone (when there are two rows)."""
    ids = np.zeros(S, dtype=np.int32)
    if G == 3 and S >= 2:
        ids[-1] = 2
    return ids


def _ranks(counts, which):
    table = {"lo": lambda n: (0, 1, (n + 1) // 2), "hi": lambda n: (n, n + 1), "mid": lambda n: ((n + 1) // 2,)}
    return np.array([table[which](int(n)) for n in counts], dtype=np.int32)


def _select(x, ranks, ids, dev, pad=3):
    """The kernel on a store with ld = C + pad (the padding holds NaN)."""
    from tecmollm import devcheck, ops
    S, C = x.shape
    store = torch.full((S, C + pad), float("nan"), device=dev)
    store[:, :C] = torch.from_numpy(x).to(dev)
    errs = devcheck.error_word(dev)
    out = ops.column_select(store, torch.from_numpy(ranks).to(dev), None if ids is None else torch.from_numpy(ids).to(dev),
                            errs.ptr(), columns=C)
    errs.post()
    return out


@pytest.mark.parametrize("C", [1, 63, 64, 65, 1620])
@pytest.mark.parametrize("S", [1, 2, 255, 256, 257, 1023, 1025])
def test_select_matches_numpy_sort(dev, S, C):
    """Every S around the waves' 32-row round and every C around the 64-column tile, ld > C; one group and three (one
    empty, one of a single row); Q = 3, 2, 1 with the ranks 0, 1, the middle, n, n + 1; every value set among the columns."""
    from tecmollm import check_device_errors
    rng = np.random.default_rng(1000 * S + C)
    for first_kind in (range(KINDS) if C == 1 else (0,)):
        x = _matrix(S, C, rng, first_kind)
        for G in (1, 3):
            ids = _group_ids(S, G)
            counts = np.bincount(ids, minlength=G)
            for which in ("lo", "hi", "mid"):
                ranks = _ranks(counts, which)
                got = _select(x, ranks, None if G == 1 else ids, dev).cpu().numpy()
                want = CR.select(x, ranks, ids, G)
                assert got.shape == want.shape == (ranks.shape[1], G, C)
                assert np.array_equal(got, want, equal_nan=True), (S, C, G, which, first_kind)
    check_device_errors()


def test_select_is_reproducible_and_skips_a_bad_group_id(dev):
    from tecmollm import TecmError, check_device_errors
    check_device_errors()
    rng = np.random.default_rng(77)
    S, C, G = 1025, 1620, 3
    x = _matrix(S, C, rng)
    ids = rng.integers(0, G, S).astype(np.int32)
    counts = np.bincount(ids, minlength=G)
    ranks = np.array([[1, (n + 1) // 2, n] for n in counts], dtype=np.int32)
    runs = [_select(x, ranks, ids, dev).view(torch.int32) for _ in range(3)]       # the bits: a selected NaN equals itself
    assert torch.isnan(runs[0].view(torch.float32)).any()
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert np.array_equal(runs[0].view(torch.float32).cpu().numpy(), CR.select(x, ranks, ids, G), equal_nan=True)
    check_device_errors()
    for bad in (G, -1):
        ids2 = ids.copy()
        ids2[500] = bad                                                    # that row leaves its group, the ranks stay
        got = _select(x, ranks, ids2, dev).cpu().numpy()
        assert np.array_equal(got, CR.select(x, ranks, ids2, G), equal_nan=True)
        with pytest.raises(TecmError, match="TECM_BAD_GROUP"):
            check_device_errors()
        check_device_errors()                                              # reported once, then clear


# ------------------------------------------------------------------------------------ scores and statistics
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
    sigma = np.abs(rng.standard_normal((S, H, I)) * 2).astype(np.float32)
    sigma[rng.random(sigma.shape) < 0.2] = 0.0                             # hits sigma_min
    sigma.reshape(-1)[0] = np.nan                                          # counts as sigma_min
    return p, t, sigma


def _layout(a, layout, dev):
    """(S, H, I) numpy -> a device view (S, H, I, 1): contiguous, or the model's permuted output (stride_h = 1, stride_i = H)."""
    d = torch.from_numpy(a).to(dev)
    if layout == "permuted":
        d = d.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    return d.unsqueeze(-1)


@pytest.mark.parametrize("H", [1, 12, 24])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 135])
def test_scores_are_the_restatement_bit_for_bit(dev, N, H):
    """Both modes x both layouts of the forecast x scaler + clip on / off x sigma on / off, hard values in every operand,
    written at row0 = 2 of a store whose other rows and padding columns hold a sentinel that must survive."""
    from tecmollm import ops
    S, row0, pad = 5, 2, 3
    rng = np.random.default_rng(100 * N + H)
    p, t, sigma = _hard(S, H, N, rng)
    td, sd = _layout(t, "contiguous", dev).squeeze(-1), torch.from_numpy(sigma).to(dev)
    for mode in CR.MODES:
        for layout in ("contiguous", "permuted"):
            pd = _layout(p, layout, dev).squeeze(-1)
            for scaler in (None, SCALER):
                for sg in (None, sigma):
                    store = torch.full((S + 4, H * N + pad), -777.0, device=dev)
                    mean, scale = scaler if scaler else (0.0, 1.0)
                    ops.conformal_scores(pd, td, store, row0, mode=mode, sigma=None if sg is None else sd, sigma_min=0.05,
                                         mean=mean, scale=scale, clip=(0.0, 200.0) if scaler else None)
                    want = CR.scores(p, t, scaler, mode, sg, 0.05)[0].reshape(S, H * N)
                    got = store.cpu().numpy()
                    what = (N, H, mode, layout, scaler, sg is not None)
                    assert np.array_equal(got[row0:row0 + S, :H * N].view(np.uint32), want.view(np.uint32)), what
                    assert np.isfinite(want).all()
                    assert (got[:row0] == -777).all() and (got[row0 + S:] == -777).all() and (got[:, H * N:] == -777).all(), what


def _assert_stats(got, want, mags, what):
    """Counts exactly; the two sums at the bar where they are finite, and the same infinity where they are not."""
    assert np.array_equal(got[:, :, :4], want[:, :, :4]), what
    g, w, m = got[:, :, 4:], want[:, :, 4:], mags[:, :, 4:]
    fin = np.isfinite(w)
    assert np.array_equal(g[~fin], w[~fin], equal_nan=True), what
    err = np.abs(g[fin] - w[fin])
    worst = float(np.max(err / np.maximum(m[fin], 1e-300))) if err.size else 0.0
    print(f"{what}: max |kernel - numpy| / sum|terms| = {worst:.3e}")
    assert np.all(err <= BAR * m[fin]), (what, worst)


def _quantiles(Gq, H, N, rng, mode, infinite):
    q_hi = np.abs(rng.standard_normal((Gq, H, N)) * 4).astype(np.float32)
    q_lo = None if mode == "absolute" else (-np.abs(rng.standard_normal((Gq, H, N)) * 4)).astype(np.float32)
    if infinite:
        q_hi[rng.random(q_hi.shape) < 0.3] = np.inf
        if q_lo is None:
            q_hi.reshape(-1)[0] = -np.inf                                  # rank 0 in the absolute mode: nothing is covered
        else:
            q_lo[rng.random(q_lo.shape) < 0.3] = -np.inf
    return q_lo, q_hi


@pytest.mark.parametrize("H", [1, 12, 24])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 135])
def test_interval_statistics_match_the_ordered_float64_restatement(dev, N, H):
    """Both modes x quantiles of one group and of every group x scaler + clip on / off, with infinite quantiles in both;
    three groups with ids out of order, group 1 never visited and pre-filled with a sentinel that must survive; two updates
    into one object, the second with a permuted forecast and a sigma; the per-sample outputs on the first."""
    from src.evaluation.metrics import IntervalMetrics
    from tecmollm import check_device_errors
    S, G, alpha = 5, 3, 0.1
    rng = np.random.default_rng(7 * N + H)
    for mode in CR.MODES:
        for Gq in (1, G):
            for scaler in (None, SCALER):
                q_lo, q_hi = _quantiles(Gq, H, N, rng, mode, infinite=True)
                q = (None if q_lo is None else torch.from_numpy(q_lo).to(dev), torch.from_numpy(q_hi).to(dev))
                im = IntervalMetrics(H, N, G, scaler, alpha, mode, dev, sigma_min=0.05)
                im.stats[1].copy_(torch.arange(H * 6 * N, device=dev, dtype=torch.float64).view(H, 6, N) + 0.5)
                sentinel = im.stats[1].clone()
                want, mags = np.zeros((G, H, 6, N)), np.zeros((G, H, 6, N))
                what = (N, H, mode, Gq, scaler)
                for update in range(2):
                    p, t, sigma = _hard(S, H, N, rng)
                    ids = np.array([2, 0, 2, 0, 2] if update == 0 else [0, 2, 2, 0, 0], dtype=np.int32)
                    sg = sigma if update == 1 else None
                    outs = im.update(_layout(p, "permuted" if update else "contiguous", dev), _layout(t, "contiguous", dev), q,
                                     torch.from_numpy(ids).to(dev), None if sg is None else torch.from_numpy(sg).to(dev),
                                     outputs=("lo", "hi", "mid") if update == 0 else ())
                    lo, hi, mid = CR.accumulate(want, mags, p, t, q_lo, q_hi, alpha, mode, ids, scaler, sg, 0.05)
                    if update == 0:
                        for name, ref in (("lo", lo), ("hi", hi), ("mid", mid)):
                            assert np.array_equal(outs[name].cpu().numpy(), ref), (what, name)
                        if scaler:
                            assert (outs["lo"] >= 0).all() and (outs["hi"] <= 200).all()
                    else:
                        assert outs == {}
                assert torch.equal(im.stats[1], sentinel), "the never-visited group was touched"
                got = im.stats.cpu().numpy()
                got[1] = want[1] = 0
                _assert_stats(got, want, mags, repr(what))
                assert got[:, :, 0].sum() == 2 * S * H * N
                assert np.array_equal(got[:, :, 1] + got[:, :, 2] + got[:, :, 3], got[:, :, 0])       # inside, under or over
                if scaler is None:
                    assert np.isinf(got[:, :, 4]).any()                    # no clip: an infinite quantile is an infinite width
                else:
                    assert np.isfinite(got).all()
    check_device_errors()


def test_interval_statistics_are_reproducible_report_bad_ids_and_serve_the_forecast_path(dev):
    from src.evaluation.metrics import IntervalMetrics
    from tecmollm import TecmError, check_device_errors, devcheck, ops
    check_device_errors()
    S, H, N, G = 16, 12, 2911, 4
    gen = torch.Generator(device=dev).manual_seed(5)
    p = torch.randn(S, N, H, device=dev, generator=gen).permute(0, 2, 1).unsqueeze(-1) * 1.5       # the model's layout
    t = torch.randn(S, H, N, 1, device=dev, generator=gen) * 1.5
    ids = torch.from_numpy(((np.arange(S) * 7) % G).astype(np.int32)).to(dev)
    q = (None, torch.rand(G, H, N, device=dev, generator=gen) * 20)
    runs = []
    for _ in range(3):
        im = IntervalMetrics(H, N, G, SCALER, 0.1, "absolute", dev)
        im.update(p, t, q, ids)
        im.update(p, t, q, ids)
        runs.append(im.stats.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert float(runs[0][:, :, 0].sum()) == 2 * S * H * N
    # the forecast path: no truth, only lo / hi are written and nothing is accumulated
    im = IntervalMetrics(H, N, G, SCALER, 0.1, "absolute", dev)
    outs = im.update(p, None, q, ids, outputs=("lo", "hi"))
    assert set(outs) == {"lo", "hi"} and float(im.stats.abs().sum()) == 0.0
    with_truth = IntervalMetrics(H, N, G, SCALER, 0.1, "absolute", dev).update(p, t, q, ids, outputs=("lo", "hi"))
    assert torch.equal(outs["lo"], with_truth["lo"]) and torch.equal(outs["hi"], with_truth["hi"])
    assert (outs["lo"] <= outs["hi"]).all() and (outs["lo"] >= 0).all() and (outs["hi"] <= 200).all()
    lo = torch.full((S, H, N), -5.0, device=dev)
    ops.interval_stats(p.squeeze(-1), None, None, q[1], None, mean=SCALER[0], scale=SCALER[1], clip=(0.0, 200.0), groups=ids,
                       num_groups=G, err_flag=devcheck.error_word(dev).ptr(), outputs={"lo": lo})
    assert torch.equal(lo, outs["lo"])
    check_device_errors()
    # a bad id: the sample is skipped everywhere, its outputs are not written, the error word says so once
    for bad in (G, -1):
        ids2 = ids.clone()
        ids2[3] = bad
        im = IntervalMetrics(H, N, G, SCALER, 0.1, "absolute", dev)
        outs2 = im.update(p, t, q, ids2, outputs=("lo",))
        assert float(im.stats[:, :, 0].sum()) == (S - 1) * H * N
        keep = torch.arange(S, device=dev) != 3
        assert torch.equal(outs2["lo"][keep], with_truth["lo"][keep])
        with pytest.raises(TecmError, match="TECM_BAD_GROUP"):
            check_device_errors()
        check_device_errors()


# ------------------------------------------------------------------------------------ calibration
@pytest.mark.parametrize("mode", CR.MODES)
def test_calibrating_and_scoring_one_split_is_exactly_self_consistent(dev, mode):
    """Calibrate on a split and score the same split: in every cell `covered` equals the number of stored scores inside
    [q_lo, q_hi], counted in numpy from the store, and that number is at least the number of ranks the interval spans.
    Equality of counts, not a statistical bound; the scores are quantised so that ties are plentiful."""
    from src.evaluation.metrics import IntervalMetrics
    from tecmollm import ConformalCalibrator, check_device_errors, conformal_ranks
    S, H, N, G, alpha = 57, 12, 65, 3, 0.2
    rng = np.random.default_rng(31)
    p = (np.round(rng.standard_normal((S, H, N)) * 4) / 4).astype(np.float32)
    t = (np.round(rng.standard_normal((S, H, N)) * 4) / 4).astype(np.float32)
    sigma = (np.round(np.abs(rng.standard_normal((S, H, N))) * 2) / 2).astype(np.float32)
    ids = rng.integers(0, G, S).astype(np.int32)
    pd, td, sd, idd = _layout(p, "permuted", dev), _layout(t, "contiguous", dev), torch.from_numpy(sigma).to(dev), torch.from_numpy(ids).to(dev)
    cal = ConformalCalibrator(H, N, S + 3, G, SCALER, mode, dev, sigma_min=0.5)
    for a, b in ((0, 20), (20, 57)):
        cal.update(pd[a:b], td[a:b], idd[a:b], sd[a:b])
    with pytest.raises(ValueError, match="do not fit"):
        cal.update(pd[:4], td[:4], idd[:4], sd[:4])
    with pytest.raises(ValueError, match="sigma"):
        cal.update(pd[:1], td[:1], idd[:1], None)
    iv = cal.fit(alpha)
    assert iv.finite and iv.counts.tolist() == np.bincount(ids, minlength=G).tolist() and iv.scaled and iv.mode == mode
    store = cal.scores[:S].cpu().numpy().reshape(S, H, N)
    assert np.array_equal(store.view(np.uint32), CR.scores(p, t, SCALER, mode, sigma, 0.5)[0].view(np.uint32))
    im = IntervalMetrics(H, N, G, SCALER, alpha, mode, dev, sigma_min=0.5)
    im.update(pd, td, iv.on(dev), idd, sd)
    covered = im.stats[:, :, 1].cpu().numpy()
    for g in range(G):
        rows = store[ids == g]
        inside = ((rows >= iv.q_lo[g]) & (rows <= iv.q_hi[g])).sum(axis=0) if mode == "signed" else (rows <= iv.q_hi[g]).sum(axis=0)
        assert np.array_equal(covered[g], inside.astype(np.float64)), g
        ranks = conformal_ranks(len(rows), alpha, mode)
        need = ranks[0] if mode == "absolute" else ranks[1] - max(ranks[0], 1) + 1
        assert (inside >= need).all() and np.array_equal(im.stats[g, :, 0].cpu().numpy(), np.full((H, N), float(len(rows))))
    # a sequence of alphas: one selection, the same intervals as one fit each
    many = cal.fit([0.1, alpha, 0.4])
    assert [m.alpha for m in many] == [0.1, 0.2, 0.4]
    assert np.array_equal(many[1].q_hi, iv.q_hi) and np.array_equal(many[1].q_lo, iv.q_lo)
    assert (many[0].q_hi >= many[1].q_hi).all() and (many[1].q_hi >= many[2].q_hi).all()
    check_device_errors()


@pytest.mark.parametrize("seed", range(2))
def test_split_conformal_coverage_on_exchangeable_scores(dev, seed):
    """The host file's case on the device: n = 199 calibration rows and 2000 test rows of |N(0, 1)| scaled per column,
    C = 256, alpha = 0.1; rank 180 of 200 gives expected coverage exactly 0.90 and the pooled coverage has a standard
    deviation of about 0.0013 (Beta(180, 20) over 256 cells), so it must lie in [0.89, 0.91]."""
    from src.evaluation.metrics import IntervalMetrics
    from tecmollm import ConformalCalibrator
    n, m, C, alpha = 199, 2000, 256, 0.1
    rng = np.random.default_rng(seed)
    col = rng.uniform(0.5, 20.0, size=C)
    calib = (np.abs(rng.standard_normal((n, C))) * col).astype(np.float32)
    test = (np.abs(rng.standard_normal((m, C))) * col).astype(np.float32)
    cal = ConformalCalibrator(1, C, n, 1, None, "absolute", dev)
    cal.update(torch.zeros(n, 1, C, device=dev), torch.from_numpy(calib).to(dev).view(n, 1, C))    # forecast 0: the score is the truth
    iv = cal.fit(alpha)
    assert np.array_equal(iv.q_hi, CR.select(calib, [[180]]).reshape(1, 1, C)) and iv.finite
    im = IntervalMetrics(1, C, 1, None, alpha, "absolute", dev)
    im.update(torch.zeros(m, 1, C, device=dev), torch.from_numpy(test).to(dev).view(m, 1, C), iv.on(dev))
    conf = im.compute()
    pooled = conf["by_group"][0]["coverage_avg"]
    print(f"seed {seed}: pooled coverage {pooled:.4f}")
    assert pooled == float((test <= iv.q_hi[0, 0]).mean())                 # the count, exactly
    assert 0.89 <= pooled <= 0.91
    assert conf["miss_below"].sum() == 0 and conf["nominal_coverage"] == 0.9


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


def test_conformal_end_to_end_on_a_tiny_model(dev, split, tmp_path):
    """12 nodes, 24 windows, batch size 5 (a ragged last batch): the first 14 windows calibrate, all are scored."""
    from src.evaluation.metrics import INTERVAL_KEYS, MAP_KEYS
    from tecmollm import conformal as CF
    from tecmollm import evaluate as E
    model, ds, ei, scaler = split
    S, N, H = len(ds), 12, 12
    cal_idx = list(range(14))
    iv = CF.calibrate_conformal(model, ds, ei, 5, alpha=0.2, scaler=scaler, order=cal_idx)
    assert model.training is False and iv.finite and iv.counts.tolist() == [14] and iv.q_hi.shape == (1, H, N)
    assert (iv.q_hi > 0).all() and np.array_equal(iv.q_lo, -iv.q_hi) and iv.scaler == scaler and not iv.scaled
    # the quantile by hand: rank ceil(15 * 0.8) = 12 of the 14 absolute errors of every cell (the same batches)
    chunks = lambda idx: [idx[a:a + 5] for a in range(0, len(idx), 5)]
    with torch.no_grad():
        parts = []
        for chunk in chunks(cal_idx):
            x, tf, y = ds.batch(chunk)
            parts.append(CR.scores(model(x, tf, ei).squeeze(-1).cpu().numpy(), y.squeeze(-1).cpu().numpy(), scaler)[0])
    assert np.array_equal(iv.q_hi[0], np.sort(np.concatenate(parts), axis=0)[11])
    # evaluate: the deterministic entries are evaluate_maps', bit for bit
    slots = (torch.arange(S, device=dev) % 3).to(torch.int32)
    want_res, want_maps = E.evaluate_maps(model, ds, ei, 5, scaler=scaler, baselines=("mean", "last"), groups=slots, num_groups=3)
    res, maps, conf = CF.evaluate_conformal(model, ds, ei, 5, iv, groups=slots, num_groups=3, baselines=("mean", "last"))
    assert list(res) == list(want_res) and list(maps) == list(want_maps)
    for name in want_res:
        for k in KEYS:
            assert res[name][k] == want_res[name][k], (name, k)
        for k in MAP_KEYS:
            assert np.array_equal(maps[name][k], want_maps[name][k], equal_nan=True), (name, k)
    assert set(conf) == set(INTERVAL_KEYS) | {"nominal_coverage", "by_group"} and conf["nominal_coverage"] == 0.8
    assert conf["count"].shape == (3, H, N) and conf["count"].sum() == S * H * N
    assert (conf["count"][0] == 8).all() and 0.0 <= conf["by_group"][1]["coverage_avg"] <= 1.0
    total = conf["coverage"] + conf["miss_below"] + conf["miss_above"]
    np.testing.assert_allclose(total, 1.0, rtol=0, atol=1e-15)
    # scoring the calibration windows alone covers at least 12 of 14 in every cell
    _, _, own = CF.evaluate_conformal(model, ds, ei, 5, iv, order=cal_idx)
    assert (own["coverage"] * 14 >= 12 - 1e-9).all() and own["count"].sum() == 14 * H * N
    # the files
    paths = CF.write_conformal(conf, str(tmp_path / "out"), grid=(3, 4))
    z = np.load(paths["npz"])
    assert sorted(z.files) == sorted(INTERVAL_KEYS + ("nominal_coverage",)) and z["coverage"].shape == (3, H, 3, 4)
    with open(paths["csv"], encoding="utf-8") as f:
        lines = f.read().splitlines()
    assert lines[0] == "group,horizon," + ",".join(CF.CSV_COLUMNS) and len(lines) == 1 + 3 * H
    # the forecast
    x, tf, y = ds.batch([20, 21])
    fc = CF.conformal_forecast(model, x, tf, ei, iv)
    assert set(fc) == {"mean", "lo", "hi"} and all(v.shape == (2, H, N) and v.is_cuda for v in fc.values())
    assert (fc["lo"] <= fc["mean"]).all() and (fc["mean"] <= fc["hi"]).all() and (fc["lo"] >= 0).all() and (fc["hi"] <= 200).all()
    with torch.no_grad():
        mid = CR.scores(model(x, tf, ei).squeeze(-1).cpu().numpy(), y.squeeze(-1).cpu().numpy(), scaler)[1]
    assert np.array_equal(fc["mean"].cpu().numpy(), mid)
    # Mondrian: three groups in one calibration equal three single-group calibrations of each group's windows
    all_idx = list(range(S))
    mon = CF.calibrate_conformal(model, ds, ei, 5, alpha=0.2, scaler=scaler, groups=slots, num_groups=3)
    assert mon.counts.tolist() == [8, 8, 8] and mon.q_hi.shape == (3, H, N)
    singles = [CF.ConformalCalibrator(H, N, S, 1, scaler, "absolute", dev) for _ in range(3)]
    with torch.no_grad():
        for chunk in chunks(all_idx):                                      # the same batches, every group's rows to its own store
            xb, tfb, yb = ds.batch(chunk)
            out = model(xb, tfb, ei)
            for g in range(3):
                rows = [j for j, i in enumerate(chunk) if i % 3 == g]
                singles[g].update(out[rows], yb[rows])
    for g in range(3):
        one = singles[g].fit(0.2)
        assert one.counts.tolist() == [8] and np.array_equal(mon.q_hi[g], one.q_hi[0]), g
    _, _, conf_m = CF.evaluate_conformal(model, ds, ei, 5, mon, groups=slots, num_groups=3)
    assert (conf_m["coverage"] * 8 >= 8 - 1 - 1e-9).all()                  # rank ceil(9 * 0.8) = 8 of 8
    fc_m = CF.conformal_forecast(model, x, tf, ei, mon, groups=slots[[20, 21]].contiguous())
    assert (fc_m["lo"] <= fc_m["hi"]).all()
    # conformalised MC dropout: reproducible under a seed, different under another, the file round trip
    a = CF.calibrate_conformal(model, ds, ei, 5, alpha=0.2, scaler=scaler, members=4, seed=3, mode="signed")
    b = CF.calibrate_conformal(model, ds, ei, 5, alpha=0.2, scaler=scaler, members=4, seed=3, mode="signed")
    c = CF.calibrate_conformal(model, ds, ei, 5, alpha=0.2, scaler=scaler, members=4, seed=4, mode="signed")
    assert model.training is False and a.scaled and a.mode == "signed" and a.finite
    assert np.array_equal(a.q_hi, b.q_hi) and np.array_equal(a.q_lo, b.q_lo) and not np.array_equal(a.q_hi, c.q_hi)
    assert (a.q_lo <= a.q_hi).all()
    loaded = CF.ConformalIntervals.load(a.save(str(tmp_path / "mc.npz")))
    assert np.array_equal(loaded.q_hi, a.q_hi) and np.array_equal(loaded.q_lo, a.q_lo) and loaded.scaled and loaded.scaler == scaler
    _, _, conf_a = CF.evaluate_conformal(model, ds, ei, 5, a, members=4, seed=3)
    _, _, conf_l = CF.evaluate_conformal(model, ds, ei, 5, loaded, members=4, seed=3)
    for k in INTERVAL_KEYS:
        assert np.array_equal(conf_a[k], conf_l[k], equal_nan=True), k
    assert (conf_a["coverage"] * S >= 22 - 1e-9).all()                     # ranks floor(25 * 0.1) = 2 .. ceil(25 * 0.9) = 23: 22 inside
    fc_a = CF.conformal_forecast(model, x, tf, ei, a, members=4, seed=3)
    assert (fc_a["lo"] <= fc_a["hi"]).all() and (fc_a["lo"] >= 0).all() and (fc_a["hi"] <= 200).all()
    with pytest.raises(ValueError, match="members"):
        CF.conformal_forecast(model, x, tf, ei, a)
    with pytest.raises(ValueError, match="members"):
        CF.evaluate_conformal(model, ds, ei, 5, iv, members=4)
