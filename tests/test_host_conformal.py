"""CPU tests of the conformal intervals' host side: `conformal_ranks` in exact arithmetic, the numpy derivation under
`IntervalMetrics`, `ConformalIntervals` and its file, `write_conformal`, the header / binding / wrappers, the entry points'
argument checks through the C ABI (no device call is reached), and the restatement of the kernels
(tests/conformal_ref.py) on its own: selection against a plain sort, and the coverage split-conformal theory promises on
exchangeable synthetic scores."""
import csv
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import conformal_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conformal_ranks_are_exact():
    from fractions import Fraction
    from tecmollm import conformal_ranks
    assert conformal_ranks(19, 0.1) == (18,)                # ceil(20 * 9 / 10): exactly 18, whatever 0.1 is in binary
    assert conformal_ranks(9, 0.1) == (9,)
    assert conformal_ranks(199, 0.1) == (180,) and conformal_ranks(2148, 0.1) == (1935,) and conformal_ranks(99, 0.05) == (95,)
    for n in range(0, 9):                                   # n < ceil(1 / alpha) - 1 = 9: no finite quantile, rank n + 1
        assert conformal_ranks(n, 0.1) == (n + 1,)
    assert conformal_ranks(9, 0.1)[0] <= 9
    assert conformal_ranks(19, 0.1, "signed") == (1, 19)
    assert conformal_ranks(18, 0.1, "signed") == (0, 19)    # the lower rank 0: -inf, and the upper n + 1: +inf
    assert conformal_ranks(39, 0.1, "signed") == (2, 38) and conformal_ranks(0, 0.5, "signed") == (0, 1)
    assert conformal_ranks(19, "0.1") == conformal_ranks(19, Fraction(1, 10)) == (18,)
    for n in (1, 7, 19, 20, 199, 2148):
        for a in (0.01, 0.05, 0.1, 0.2, 0.5):
            fr = Fraction(str(a))
            k, = conformal_ranks(n, a)
            assert k - 1 < (n + 1) * (1 - fr) <= k and 1 <= k <= n + 1
            lo, hi = conformal_ranks(n, a, "signed")
            assert lo <= (n + 1) * fr / 2 < lo + 1 and hi - 1 < (n + 1) * (1 - fr / 2) <= hi and 0 <= lo < hi <= n + 1
    for bad in (0, 1, -0.1, 1.5):
        with pytest.raises(ValueError):
            conformal_ranks(10, bad)
    with pytest.raises(ValueError):
        conformal_ranks(-1, 0.1)
    with pytest.raises(ValueError):
        conformal_ranks(10, 0.1, "both")


def test_derive_intervals_on_hand_built_statistics():
    from src.evaluation.metrics import INTERVAL_KEYS, IntervalMetrics, derive_intervals
    assert INTERVAL_KEYS == ("count", "coverage", "miss_below", "miss_above", "interval_width", "interval_score")
    #       count covered below above Swidth SWinkler
    row = [8.0, 6.0, 1.0, 1.0, 20.0, 36.0]
    d = derive_intervals(np.array([row, [0.0] * 6]))
    assert set(d) == set(INTERVAL_KEYS)
    want = {"count": 8.0, "coverage": 0.75, "miss_below": 0.125, "miss_above": 0.125, "interval_width": 2.5,
            "interval_score": 4.5}
    for k, v in want.items():
        assert d[k][0] == v, k
        if k != "count":
            assert np.isnan(d[k][1]), k
    assert d["count"][1] == 0
    with pytest.raises(ValueError):
        derive_intervals(np.zeros((2, 5)))
    im = IntervalMetrics(2, 3, 2, None, 0.2, "signed", device="cpu")
    assert im.stats.shape == (2, 2, 6, 3) and im.stats.dtype == torch.float64 and im.nominal_coverage == 0.8
    im.stats[0, :, :, :] = torch.tensor(row, dtype=torch.float64).view(1, 6, 1)
    assert im.merge_() is im                                               # no process group: a no-op
    out = im.compute()
    assert set(out) == set(INTERVAL_KEYS) | {"nominal_coverage", "by_group"} and out["nominal_coverage"] == 0.8
    for k, v in want.items():
        assert out[k].shape == (2, 2, 3) and (out[k][0] == v).all()
        assert np.isnan(out[k][1]).all() or k == "count"
    pooled = out["by_group"][0]
    assert pooled["coverage_by_horizon"] == [0.75, 0.75] and pooled["count_by_horizon"] == [24.0, 24.0]
    assert pooled["interval_score_avg"] == 4.5 and np.isnan(out["by_group"][1]["coverage_avg"])
    im.reset()
    assert float(im.stats.abs().sum()) == 0.0
    for bad in (dict(alpha=0.0), dict(alpha=1.0), dict(mode="both"), dict(num_groups=0)):
        kw = dict(num_horizons=2, num_nodes=3, num_groups=1, scaler=None, alpha=0.1, mode="absolute", device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError):
            IntervalMetrics(**kw)


def _intervals(mode="signed", G=2, H=3, N=5):
    from tecmollm import ConformalIntervals
    rng = np.random.default_rng(4)
    q_hi = np.abs(rng.standard_normal((G, H, N))).astype(np.float32)
    q_hi[1, 0, 0] = np.inf
    q_lo = -q_hi if mode == "absolute" else -np.abs(rng.standard_normal((G, H, N))).astype(np.float32)
    return ConformalIntervals(q_lo, q_hi, 0.1, mode, [17, 3], 0.002, mode == "signed", 21.5, 9.25, True)


@pytest.mark.parametrize("mode", CR.MODES)
def test_conformal_intervals_round_trip_through_a_file(tmp_path, mode):
    from tecmollm import ConformalIntervals
    a = _intervals(mode)
    path = a.save(str(tmp_path / "intervals.npz"))
    assert os.path.basename(path) == "intervals.npz"
    with np.load(path, allow_pickle=False) as z:                           # numpy arrays only: loads without pickle
        assert sorted(z.files) == sorted(["q_lo", "q_hi", "alpha", "mode", "counts", "sigma_min", "scaled", "mean", "scale", "clip"])
    b = ConformalIntervals.load(path)
    assert np.array_equal(a.q_lo, b.q_lo) and np.array_equal(a.q_hi, b.q_hi) and b.q_hi.dtype == np.float32
    assert (b.alpha, b.mode, b.sigma_min, b.scaled, b.mean, b.scale, b.clip) == (0.1, mode, 0.002, mode == "signed", 21.5, 9.25, True)
    assert b.counts.tolist() == [17, 3] and b.num_groups == 2 and b.scaler == (21.5, 9.25)
    assert not b.finite                                                    # one cell of group 1 had too few samples
    b.q_hi[1, 0, 0] = 1.0
    b.q_lo[1, 0, 0] = -1.0
    assert b.finite
    lo, hi = b.on("cpu")
    assert (lo is None) == (mode == "absolute") and hi.shape == (2, 3, 5) and hi.is_contiguous()
    assert ConformalIntervals(a.q_lo, a.q_hi, 0.1, mode, [1, 1]).scaler is None
    with pytest.raises(ValueError):
        ConformalIntervals(a.q_lo, a.q_hi, 0.1, "both", [1, 1])
    with pytest.raises(ValueError):
        ConformalIntervals(a.q_lo[0], a.q_hi[0], 0.1, mode, [1])
    with pytest.raises(ValueError):
        ConformalIntervals(a.q_lo, a.q_hi, 0.1, mode, [1, 1, 1])


@pytest.mark.parametrize("grid", [None, (2, 3)])
def test_write_conformal_round_trips(tmp_path, grid):
    from src.evaluation.metrics import INTERVAL_KEYS, IntervalMetrics
    from tecmollm import write_conformal
    from tecmollm.conformal import CSV_COLUMNS
    G, H, I = 2, 3, 6
    rng = np.random.default_rng(8)
    pred, true = (rng.standard_normal((9, H, I)).astype(np.float32) for _ in range(2))
    q_hi = np.full((1, H, I), 1.25, dtype=np.float32)
    stats, mags = np.zeros((G, H, 6, I)), np.zeros((G, H, 6, I))
    CR.accumulate(stats, mags, pred, true, None, q_hi, 0.1)               # group 1 is never visited
    im = IntervalMetrics(H, I, G, None, 0.1, "absolute", device="cpu")
    im.stats.copy_(torch.from_numpy(stats))
    conf = im.compute()
    assert conf["count"][0].sum() == 9 * H * I and 0.5 < conf["by_group"][0]["coverage_avg"] < 1.0
    paths = write_conformal(conf, str(tmp_path / "out"), grid=grid)
    assert sorted(os.listdir(tmp_path / "out")) == ["conformal_by_horizon.csv", "conformal_maps.npz"]
    z = np.load(paths["npz"])
    assert sorted(z.files) == sorted(INTERVAL_KEYS + ("nominal_coverage",)) and float(z["nominal_coverage"]) == 0.9
    for k in INTERVAL_KEYS:
        assert z[k].shape == ((G, H, I) if grid is None else (G, H, 2, 3))
        assert np.array_equal(z[k].reshape(G, H, I), conf[k], equal_nan=True)
    with open(paths["csv"], newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["group", "horizon"] + list(CSV_COLUMNS)
    assert [(r[0], r[1]) for r in rows[1:]] == [(str(g), str(h)) for g in range(G) for h in range(H)]
    for r in rows[1:]:
        pooled = conf["by_group"][int(r[0])]
        for cell, k in zip(r[2:], CSV_COLUMNS):
            want = conf["nominal_coverage"] if k == "nominal_coverage" else pooled[f"{k}_by_horizon"][int(r[1])]
            assert float(cell) == want or (np.isnan(float(cell)) and np.isnan(want)), (r, k)
    with pytest.raises(ValueError):
        write_conformal(conf, str(tmp_path / "bad"), grid=(4, 2))


def _struct_names(header, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"[\s*](\w+)\s*[,;]", body)


def test_header_binding_and_wrappers_agree_on_the_new_symbols():
    import tecmollm
    from tecmollm import _lib, ops
    header = open(os.path.join(ROOT, "include", "tecmollm.h")).read()
    for define, value in (("TECM_CONF_ABS", 0), ("TECM_CONF_SIGNED", 1), ("TECM_INTERVAL_STATS", 6), ("TECM_SELECT_MAX_Q", 8)):
        assert f"#define {define} {value}" in header and getattr(_lib, define) == value
    assert CR.STATS == 6 and ops.CONFORMAL_MODES == {"absolute": 0, "signed": 1} and tuple(ops.CONFORMAL_MODES) == CR.MODES
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for fn, struct, arg in (("tecm_conformal_scores", "TecmConformalScores", "c"), ("tecm_column_select", "TecmColumnSelect", "c"),
                            ("tecm_interval_stats", "TecmIntervalStats", "c")):
        assert f"int {fn}(const {struct}* {arg}, void* stream);" in header
        assert fn in _lib.EXPORTS and hasattr(handle, fn)
        assert _struct_names(header, struct) == [f[0] for f in getattr(_lib, struct)._fields_], struct
    assert ctypes.sizeof(_lib.TecmConformalScores) == 8 * 12 + 8 + 4 + 4 + 8 + 16 + 16 + 8 * 3
    assert ctypes.sizeof(_lib.TecmColumnSelect) == 8 * 4 + 8 * 2 + 4 + 4 + 8 * 2
    assert ctypes.sizeof(_lib.TecmIntervalStats) == 8 * 12 + 8 + 4 + 4 + 8 + 16 + 16 + 8 * 2 + 4 + 4 + 8 + 8 * 3 + 8 * 3 + 8 * 3
    # additive entry points: the version stays (the binding and the header move together when a layout changes)
    assert _lib.ABI_VERSION == int(re.search(r"#define\s+TECM_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.lib().tecm_abi_version()
    assert "conformal.hip" in __import__("__graft_entry__").SOURCES
    rules = __import__("__graft_entry__").SPILL_CEILINGS["conformal.hip"]
    assert sorted(r[0] for r in rules) == ["column_select_kernel", "conformal_scores_kernel", "interval_stats_kernel"]
    assert all(r[1:] == ("ScratchSize [bytes/lane]", 0) for r in rules)
    for name in ("conformal_ranks", "ConformalCalibrator", "ConformalIntervals", "calibrate_conformal", "conformal_forecast",
                 "evaluate_conformal", "write_conformal"):
        assert name in tecmollm.__all__ and callable(getattr(tecmollm, name))
    assert ops.INTERVAL_OUTPUTS == ("lo", "hi", "mid")


def _buf():
    buf = (ctypes.c_double * 8)()                                          # a real, aligned host address: never dereferenced
    return buf, ctypes.addressof(buf)


def _scores_descriptor(**over):
    from tecmollm import _lib
    buf, a = _buf()
    f = dict(pred=a, p_stride_s=1, p_stride_h=1, p_stride_i=1, target=a, t_stride_s=1, t_stride_h=1, t_stride_i=1, sigma=None,
             S=1, H=1, mode=0, I=1, mean=0.0, scale=1.0, clip=0, sigma_min=1e-3, scores=a, ld=1, row0=0)
    f.update(over)
    d = _lib.TecmConformalScores(**f)
    d._keep = buf
    return d


def _select_descriptor(**over):
    from tecmollm import _lib
    buf, a = _buf()
    f = dict(x=a, ld=1, S=1, C=1, group=None, ranks=a, G=1, Q=1, out=a, err_flag=a)
    f.update(over)
    d = _lib.TecmColumnSelect(**f)
    d._keep = buf
    return d


def _stats_descriptor(**over):
    from tecmollm import _lib
    buf, a = _buf()
    f = dict(pred=a, p_stride_s=1, p_stride_h=1, p_stride_i=1, target=a, t_stride_s=1, t_stride_h=1, t_stride_i=1, sigma=None,
             S=1, H=1, mode=0, I=1, mean=0.0, scale=1.0, clip=0, sigma_min=1e-3, q_lo=None, q_hi=a, Gq=1, G=1, alpha=0.1,
             stats=a, group=None, err_flag=a)
    f.update(over)
    d = _lib.TecmIntervalStats(**f)
    d._keep = buf
    return d


@pytest.mark.parametrize("make, fn, over, text", [
    (_scores_descriptor, "tecm_conformal_scores", dict(pred=None), b"null pointer"),
    (_scores_descriptor, "tecm_conformal_scores", dict(scores=None), b"null pointer"),
    (_scores_descriptor, "tecm_conformal_scores", dict(S=0), b"bad shape"),
    (_scores_descriptor, "tecm_conformal_scores", dict(mode=2), b"unknown mode"),
    (_scores_descriptor, "tecm_conformal_scores", dict(H=2, I=3, ld=5), b"ld >= H * I"),
    (_scores_descriptor, "tecm_conformal_scores", dict(row0=-1), b"row0 >= 0"),
    (_scores_descriptor, "tecm_conformal_scores", dict(scale=0.0), b"scale must be non-zero"),
    (_scores_descriptor, "tecm_conformal_scores", dict(sigma=1, sigma_min=0.0), b"sigma_min > 0"),
    (_select_descriptor, "tecm_column_select", dict(x=None), b"null pointer"),
    (_select_descriptor, "tecm_column_select", dict(err_flag=None), b"null pointer"),
    (_select_descriptor, "tecm_column_select", dict(S=0), b"0 < S < 2^31"),
    (_select_descriptor, "tecm_column_select", dict(S=1 << 31, ld=1), b"0 < S < 2^31"),
    (_select_descriptor, "tecm_column_select", dict(Q=0), b"outside [1, 8]"),
    (_select_descriptor, "tecm_column_select", dict(Q=9), b"outside [1, 8]"),
    (_select_descriptor, "tecm_column_select", dict(G=0), b"[1, 65535]"),
    (_select_descriptor, "tecm_column_select", dict(G=65536), b"[1, 65535]"),
    (_select_descriptor, "tecm_column_select", dict(C=4, ld=3), b"ld >= C"),
    (_stats_descriptor, "tecm_interval_stats", dict(q_hi=None), b"null pointer"),
    (_stats_descriptor, "tecm_interval_stats", dict(stats=None), b"a target needs stats"),
    (_stats_descriptor, "tecm_interval_stats", dict(target=None), b"needs a per-sample output"),
    (_stats_descriptor, "tecm_interval_stats", dict(mode=1), b"needs q_lo"),
    (_stats_descriptor, "tecm_interval_stats", dict(G=3, Gq=2), b"Gq must be 1 or G"),
    (_stats_descriptor, "tecm_interval_stats", dict(alpha=0.0), b"alpha must lie in (0, 1)"),
    (_stats_descriptor, "tecm_interval_stats", dict(alpha=1.0), b"alpha must lie in (0, 1)"),
    (_stats_descriptor, "tecm_interval_stats", dict(G=65536, Gq=65536), b"<= 65535"),
    (_stats_descriptor, "tecm_interval_stats", dict(scale=0.0), b"scale must be non-zero"),
])
def test_the_launchers_reject_bad_descriptors_before_any_device_call(make, fn, over, text):
    from tecmollm import _lib
    d = make(**over)
    rc = getattr(_lib.lib(), fn)(ctypes.byref(d), None)
    assert rc == -1, (over, rc)                                            # TECM_E_ARG
    assert text in _lib.lib().tecm_last_error(), (over, _lib.lib().tecm_last_error())


def test_the_launchers_reject_a_null_descriptor_and_misaligned_pointers():
    from tecmollm import _lib
    for fn, make, field in (("tecm_conformal_scores", _scores_descriptor, "scores"), ("tecm_column_select", _select_descriptor, "out"),
                            ("tecm_interval_stats", _stats_descriptor, "stats")):
        assert getattr(_lib.lib(), fn)(None, None) == -1 and b"null descriptor" in _lib.lib().tecm_last_error()
        d = make()
        setattr(d, field, getattr(d, field) + 2)
        assert getattr(_lib.lib(), fn)(ctypes.byref(d), None) == -2, fn    # TECM_E_ALIGN
        assert b"aligned" in _lib.lib().tecm_last_error()


def test_the_restated_selection_is_a_plain_sort_with_numpys_order():
    x = np.array([[3.0, np.nan], [-0.0, -np.inf], [0.0, np.inf], [-2.0, -np.nan], [np.inf, 1.0]], dtype=np.float32)
    out = CR.select(x, [[0, 1, 2, 3, 5, 6]])
    assert out.shape == (6, 1, 2)
    assert np.array_equal(out[:, 0, 0], np.array([-np.inf, -2, 0, 0, np.inf, np.inf], dtype=np.float32))
    assert np.array_equal(out[:, 0, 1], np.array([-np.inf, -np.inf, 1, np.inf, np.nan, np.inf], dtype=np.float32), equal_nan=True)
    # groups: ids out of order, one empty group, one row in no group
    ids = np.array([2, 0, 2, 7, 0])
    out = CR.select(x[:, :1], [[1, 2], [1, 0], [2, 3]], ids, 3)
    assert out[:, 0, 0].tolist() == [-0.0, np.inf] and out[:, 1, 0].tolist() == [np.inf, -np.inf]
    assert out[:, 2, 0].tolist() == [3.0, np.inf]


@pytest.mark.parametrize("seed", range(5))
def test_split_conformal_coverage_on_exchangeable_scores(seed):
    """n = 199 calibration rows and 2000 test rows of |N(0, 1)| scaled per column, C = 256, alpha = 0.1: the rank is 180 of
    200, so a test score is covered with probability exactly 180 / 200 = 0.90 and the coverage of a column is Beta(180, 20),
    standard deviation sqrt(0.9 * 0.1 / 201) = 0.021; pooled over 256 independent columns of 2000 test rows each that is
    0.021 / 16 = 0.0013 (the binomial noise of the test rows adds sqrt(0.09 / 512000) = 0.0004).  [0.89, 0.91] is seven such
    deviations wide on either side."""
    from tecmollm import conformal_ranks
    n, m, C, alpha = 199, 2000, 256, 0.1
    rng = np.random.default_rng(seed)
    col = rng.uniform(0.5, 20.0, size=C)
    cal = (np.abs(rng.standard_normal((n, C))) * col).astype(np.float32)
    test = (np.abs(rng.standard_normal((m, C))) * col).astype(np.float32)
    k, = conformal_ranks(n, alpha)
    assert k == 180
    q = CR.select(cal, [[k]])[0, 0]
    assert np.isfinite(q).all() and ((cal <= q).sum(axis=0) >= k).all()
    pooled = float((test <= q).mean())
    print(f"seed {seed}: pooled coverage {pooled:.4f}")
    assert 0.89 <= pooled <= 0.91
    # the same through the restated statistics: truth = score, forecast = 0, no scaler
    stats, mags = np.zeros((1, 1, 6, C)), np.zeros((1, 1, 6, C))
    CR.accumulate(stats, mags, np.zeros((m, 1, C), dtype=np.float32), test.reshape(m, 1, C), None, q.reshape(1, 1, C), alpha)
    assert stats[0, 0, 0].sum() == m * C and stats[0, 0, 1].sum() / (m * C) == pooled
    assert np.array_equal(stats[0, 0, 1] + stats[0, 0, 2] + stats[0, 0, 3], stats[0, 0, 0]) and stats[0, 0, 2].sum() == 0
