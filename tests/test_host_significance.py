"""CPU tests of the significance feature's host side: the bootstrap's row sequence, the interval ranks, Student's t tail,
the Diebold-Mariano statistic by hand, the header / binding / build entries, what the two launchers refuse through the C ABI
(no device call is reached), and the size of both methods on autocorrelated series, on the restatement alone
(tests/significance_ref.py)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import significance_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------ row sequence
@pytest.mark.parametrize("S, L", [(1, 1), (7, 1), (7, 2), (7, 3), (7, 7), (7, 12), (64, 5), (257, 32)])
def test_row_sequence_has_ceil_blocks_truncates_and_wraps(S, L):
    from tecmollm.significance import bootstrap_rows, draw_starts
    K = -(-S // L)
    starts = draw_starts(S, L, 3, seed=5)
    assert starts.shape == (3, K) and starts.dtype == torch.int32 and not starts.is_cuda
    assert torch.equal(starts, draw_starts(S, L, 3, seed=5)) and (S < 3 or not torch.equal(starts, draw_starts(S, L, 3, seed=6)))
    for st in starts.tolist():
        rows = bootstrap_rows(st, S, L)
        assert rows == SR.bootstrap_rows(st, S, L) and len(rows) == S and all(0 <= r < S for r in rows)
        for t, r in enumerate(rows):                                       # consecutive inside a block, modulo S
            assert r == (st[t // L] + t % L) % S
            if t % L:
                assert r == (rows[t - 1] + 1) % S
    with pytest.raises(ValueError):
        bootstrap_rows([0] * (K + 1), S, L)
    with pytest.raises(ValueError):
        bootstrap_rows([0] * K, S, 0)


def test_row_sequence_special_cases():
    from tecmollm.significance import bootstrap_rows
    for S, L in ((7, 7), (7, 12), (1, 1)):                                 # L >= S with start 0: the windows in order
        assert bootstrap_rows([0], S, L) == list(range(S))
    assert bootstrap_rows([5], 7, 9) == [5, 6, 0, 1, 2, 3, 4]              # one wrap
    assert bootstrap_rows([3, 3, 0, 6, 3], 5, 1) == [3, 3, 0, 1, 3]        # L = 1: an iid resample (6 mod 5 = 1)
    assert bootstrap_rows([4, 1, 6], 7, 3) == [4, 5, 6, 1, 2, 3, 6]        # the last block truncated to one window
    # the plain totals, exactly: a sequential sum of the windows in order
    rng = np.random.default_rng(0)
    table = rng.standard_normal((2, 9, 5))
    want = np.zeros((2, 5))
    for s in range(9):
        want += table[:, s]
    for L in (9, 14):
        assert np.array_equal(SR.bootstrap_sums(table, [[0]], L)[0, :, 0], want)
    # groups: an empty group gives zeros, a bad id and a bad start are skipped
    ids = np.array([0, 2, 2, 0, 0, 0, 7, 0, 0])
    got = SR.bootstrap_sums(table, [[0, 3, 9]], 3, ids, 3)[0]
    assert (got[:, 1] == 0).all() and np.array_equal(got[:, 2], table[:, 1] + table[:, 2])
    assert np.array_equal(got[:, 0], (table[:, 0] + table[:, 3]) + table[:, 4] + table[:, 5])


# ------------------------------------------------------------------------------------ ranks, t tail, DM
def test_interval_ranks_round_outward():
    from fractions import Fraction
    from tecmollm.significance import interval_ranks, percentile_interval
    assert interval_ranks(1, 0.9) == (0, 0) and interval_ranks(2, 0.9) == (0, 1)
    assert interval_ranks(10, 0.9) == (0, 9) and interval_ranks(1000, 0.9) == (49, 950)
    assert interval_ranks(21, 0.9) == (1, 19) and interval_ranks(21, Fraction(9, 10)) == (1, 19)    # exact products stay
    for R in (1, 2, 10, 21, 300, 1000):
        assert interval_ranks(R, 0.9) == SR.interval_ranks(R, 0.9)
        lo, hi = interval_ranks(R, 0.9)
        assert lo <= 0.05 * (R - 1) < lo + 1 and hi - 1 < 0.95 * (R - 1) <= hi + 1e-9 and 0 <= lo <= hi <= R - 1
    for bad in (0, 1, 1.5):
        with pytest.raises(ValueError):
            interval_ranks(10, bad)
    v = np.array([[3.0, np.nan, np.nan], [1.0, 5.0, np.nan], [2.0, np.nan, np.nan], [0.0, 4.0, np.nan]])
    lo, hi, nan = percentile_interval(v, 0.5)                              # ranks of 4: (0, 3); of 2: (0, 1)
    assert lo.tolist()[:2] == [0.0, 4.0] and hi.tolist()[:2] == [3.0, 5.0] and nan.tolist() == [0, 2, 4]
    assert np.isnan(lo[2]) and np.isnan(hi[2])
    for col in range(2):
        assert SR.interval(v[:, col], 0.5) == (lo[col], hi[col], nan[col])


# 2 * sf(t; df) to full double precision; each rounds to the ten decimals quoted beside it
T_TAIL = [(2.0, 10, 0.07338803477074037, 0.0733880348), (1.0, 3, 0.39100221895577064, 0.3910022190),
          (2.5, 2148, 0.012493367226172716, 0.0124933672), (0.5, 1, 0.7048327646991335, 0.7048327647)]


@pytest.mark.parametrize("t, df, want, quoted", T_TAIL)
def test_t_tail_against_constants(t, df, want, quoted):
    from tecmollm.significance import betainc, t_two_sided
    assert round(want, 10) == quoted
    got = t_two_sided(t, df)
    print(f"2 sf({t}; {df}) = {got!r}, restated {SR.t_two_sided(t, df)!r}")
    assert abs(got - want) <= 1e-9 * want and t_two_sided(-t, df) == got
    assert abs(SR.t_two_sided(t, df) - want) <= 1e-9 * want               # the finite series agrees with the beta function
    assert betainc(2.0, 3.0, 0.0) == 0.0 and betainc(2.0, 3.0, 1.0) == 1.0
    assert abs(betainc(2.0, 3.0, 0.4) - 0.5248) < 1e-14                   # I_x(2, 3) = 6x^2 - 8x^3 + 3x^4
    assert math.isnan(t_two_sided(math.nan, 5)) and t_two_sided(math.inf, 5) == 0.0 and t_two_sided(0.0, 5) == 1.0


def test_dm_by_hand_on_six_points():
    """d = 1, 2, 3, 1, 2, 6: dbar = 2.5, c = -1.5, -.5, .5, -1.5, -.5, 3.5; gamma_0 = 17.5 / 6, gamma_1 = (0.75 - 0.25 - 0.75 +
    0.75 - 1.75) / 6 = -1.25 / 6; q = 1: V = (17.5 - 1.25) / 6 = 16.25 / 6; HLN with h = 2: (6 + 1 - 4 + 2 / 6) / 6 = 10 / 18;
    DM = 2.5 / sqrt(16.25 / 36) * sqrt(10 / 18)."""
    from tecmollm.significance import dm_statistic, t_two_sided
    d = [1.0, 2.0, 3.0, 1.0, 2.0, 6.0]
    r = dm_statistic(d, 1)
    want = 2.5 / math.sqrt(16.25 / 36.0) * math.sqrt(10.0 / 18.0)
    assert r["lags"] == 1 and r["n"] == 6 and r["mean"] == 2.5
    assert abs(r["variance"] - 16.25 / 6.0) < 1e-14 and abs(r["stat"] - want) < 1e-13
    assert r["p"] == t_two_sided(r["stat"], 5) and 0.0 < r["p"] < 0.1
    stat, p = SR.dm(d, 1)
    assert abs(stat - r["stat"]) < 1e-13 and abs(p - r["p"]) < 1e-12
    r0 = dm_statistic(d, 0)                                                # q = 0: the naive test, HLN factor (6 - 1) / 6
    assert abs(r0["stat"] - 2.5 / math.sqrt(17.5 / 36.0) * math.sqrt(5.0 / 6.0)) < 1e-13
    assert dm_statistic(d, 99)["lags"] == 5                                # capped at S - 1
    for series in ([0.3] * 6, [0.0] * 6, [1.0], []):                       # constant, a against a, too short
        r = dm_statistic(series, 1)
        assert math.isnan(r["stat"]) and math.isnan(r["p"])
        assert all(math.isnan(v) for v in SR.dm(series, 1))
    assert math.isnan(dm_statistic([1.0, math.nan, 2.0], 0)["stat"])


def test_diebold_mariano_and_intervals_from_a_hand_built_table(tmp_path):
    """`WindowScores` on the CPU (no launch): the loss differential comes from columns 7 / 6 over column 0; a forecast
    against itself and a constant differential give NaN; save / load round trip."""
    from tecmollm.significance import WindowScores, default_block_len, default_lags, diebold_mariano, dm_statistic
    S, H = 6, 2
    ws = WindowScores(S, H, ["A", "B"], (21.5, 9.25), "cpu", L_in=4, L_out=2, stride=1)
    assert ws.table.shape == (2, S, H, 8) and ws.table.dtype == torch.float64 and float(ws.table.abs().sum()) == 0.0
    d = np.array([1.0, 2.0, 3.0, 1.0, 2.0, 6.0])
    ws.table[:, :, :, 0] = 4.0                                             # four nodes
    ws.table[0, :, 0, 7] = torch.from_numpy(4.0 * (d + 10.0))              # se of A at horizon 0: d + 10; of B: 10
    ws.table[1, :, 0, 7] = 40.0
    ws.table[0, :, 1, 6] = 8.0                                             # ae at horizon 1: equal
    ws.table[1, :, 1, 6] = 8.0
    r = diebold_mariano(ws, "A", "B", "se", lags=1)
    assert r["n"] == S and r["lags"] == 1 and r["loss"] == "se"
    assert r["stat"][0] == dm_statistic(d, 1)["stat"] and math.isnan(r["stat"][1])
    assert r["stat_pooled"] == dm_statistic(d / 2, 1)["stat"]              # pooled: d averaged over the two horizons
    assert np.isnan(diebold_mariano(ws, "A", "B", "ae", lags=1)["stat"]).all()
    same = diebold_mariano(ws, "A", "A", "se")
    assert np.isnan(same["stat"]).all() and math.isnan(same["stat_pooled"]) and same["lags"] == default_lags(S, 2, 1)
    by = diebold_mariano(ws, "A", "B", "se", lags=0, groups=torch.tensor([0, 1, 0, 1, 0, 9], dtype=torch.int32), num_groups=2)
    assert [g["n"] for g in by] == [3, 2] and by[0]["stat"][0] == dm_statistic(d[[0, 2, 4]], 0)["stat"]
    ws.table[:, 3] = 0.0                                                   # a window never written is left out
    assert diebold_mariano(ws, "A", "B", "se", lags=1)["n"] == S - 1
    with pytest.raises(ValueError):
        diebold_mariano(ws, "A", "B", "huber")
    with pytest.raises(KeyError):
        diebold_mariano(ws, "A", "C")
    assert default_block_len(2149, 48, 12, 1) == 120 and default_block_len(24, 16, 12, 1) == 3
    assert default_block_len(2149, 48, 12, 12) == 10 and default_block_len(5, 16, 12) == 1
    assert default_lags(2149, 12, 1) == 11 and default_lags(2149, 12, 12) == 7 and default_lags(100, 1, 1) == 4
    path = ws.save(str(tmp_path / "scores.npz"))
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["clip", "mean", "names", "scale", "table", "window"]
    back = WindowScores.load(path, "cpu")
    assert torch.equal(back.table, ws.table) and back.names == ["A", "B"] and back.scaler == (21.5, 9.25)
    assert (back.L_in, back.L_out, back.stride) == (4, 2, 1)
    with pytest.raises(ValueError):
        WindowScores(0, 2, ["A"], None, "cpu")
    with pytest.raises(ValueError):
        WindowScores(3, 2, ["A", "A"], None, "cpu")


# ------------------------------------------------------------------------------------ header, binding, build
def _struct_names(header, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"[\s*](\w+)\s*[,;]", body)


def test_header_binding_and_build_agree_on_the_new_symbols():
    import tecmollm
    from tecmollm import _lib, devcheck
    header = open(os.path.join(ROOT, "include", "tecmollm.h")).read()
    for define, value in (("TECM_BAD_ROW", 32), ("TECM_BAD_START", 64)):
        assert f"#define {define} {value}" in header and getattr(_lib, define) == value
    assert (devcheck.BAD_ROW, devcheck.BAD_START) == (32, 64)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for fn, struct, arg in (("tecm_metrics_window", "TecmMetricsWindow", "m"), ("tecm_block_bootstrap", "TecmBlockBootstrap", "b")):
        assert f"int {fn}(const {struct}* {arg}, void* stream);" in header
        assert fn in _lib.EXPORTS and hasattr(handle, fn)
        assert _struct_names(header, struct) == [f[0] for f in getattr(_lib, struct)._fields_], struct
    assert ctypes.sizeof(_lib.TecmMetricsWindow) == ctypes.sizeof(_lib.TecmMetrics) - 8 + 8 * 5
    assert ctypes.sizeof(_lib.TecmBlockBootstrap) == 8 * 3 + 8 * 3 + 8 + 4 + 4 + 8 + 8 * 3 + 8 * 2
    assert _lib.ABI_VERSION == int(re.search(r"#define\s+TECM_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.lib().tecm_abi_version()
    entry = __import__("__graft_entry__")
    assert "significance.hip" in entry.SOURCES
    rules = entry.SPILL_CEILINGS["significance.hip"]
    assert sorted(r[0] for r in rules) == ["block_bootstrap_kernel", "metrics_window_kernel"]
    assert all(r[1:] == ("ScratchSize [bytes/lane]", 0) for r in rules)
    for name in ("WindowScores", "score_windows", "block_bootstrap", "bootstrap_intervals", "diebold_mariano",
                 "evaluate_significance", "write_significance"):
        assert name in tecmollm.__all__ and callable(getattr(tecmollm, name))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "tecm_metrics_window" in integration and "tecm_block_bootstrap" in integration


def _buf():
    buf = (ctypes.c_double * 8)()                                          # a real, aligned host address: never dereferenced
    return buf, ctypes.addressof(buf)


def _window_descriptor(**over):
    from tecmollm import _lib
    buf, a = _buf()
    f = dict(pred=a, p_stride_s=1, p_stride_h=1, p_stride_i=1, target=a, t_stride_s=1, t_stride_h=1, t_stride_i=1,
             S=1, H=1, I=1, mean=0.0, scale=1.0, clip=0, table=a, table_rows=1, rows=None, row0=0, err_flag=a)
    f.update(over)
    d = _lib.TecmMetricsWindow(**f)
    d._keep = buf
    return d


def _boot_descriptor(**over):
    from tecmollm import _lib
    buf, a = _buf()
    f = dict(table=a, stride_m=8, stride_s=1, M=1, S=8, W=1, group=None, G=1, starts=a, R=1, K=2, L=4, out=a, err_flag=a)
    f.update(over)
    d = _lib.TecmBlockBootstrap(**f)
    d._keep = buf
    return d


@pytest.mark.parametrize("make, fn, over, text", [
    (_window_descriptor, "tecm_metrics_window", dict(pred=None), b"null pointer"),
    (_window_descriptor, "tecm_metrics_window", dict(target=None), b"null pointer"),
    (_window_descriptor, "tecm_metrics_window", dict(table=None), b"null pointer"),
    (_window_descriptor, "tecm_metrics_window", dict(err_flag=None), b"null pointer"),
    (_window_descriptor, "tecm_metrics_window", dict(S=0), b"bad shape"),
    (_window_descriptor, "tecm_metrics_window", dict(H=0), b"bad shape"),
    (_window_descriptor, "tecm_metrics_window", dict(I=-1), b"bad shape"),
    (_window_descriptor, "tecm_metrics_window", dict(table_rows=0), b"bad shape"),
    (_window_descriptor, "tecm_metrics_window", dict(S=1 << 31), b"S must be < 2^31"),
    (_window_descriptor, "tecm_metrics_window", dict(H=4 * 65535 + 1), b"ceil(H / 4) <= 65535"),
    (_window_descriptor, "tecm_metrics_window", dict(table_rows=1 << 62), b"do not fit 64-bit addressing"),
    (_window_descriptor, "tecm_metrics_window", dict(scale=0.0), b"scale must be non-zero"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(table=None), b"null pointer"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(starts=None), b"null pointer"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(out=None), b"null pointer"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(err_flag=None), b"null pointer"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(M=0), b"bad shape"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(W=0), b"bad shape"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(R=0), b"bad shape"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(S=0), b"0 < S < 2^31"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(S=1 << 31), b"0 < S < 2^31"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(L=0), b"1 <= block_len"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(K=3), b"K must be ceil(S / block_len)"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(L=3, K=2), b"K must be ceil(S / block_len)"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(G=0), b"G outside [1, 65535]"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(G=65536), b"G outside [1, 65535]"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(W=400, stride_s=400, G=16, M=586), b"must be <= 65535"),
    (_boot_descriptor, "tecm_block_bootstrap", dict(W=4, stride_s=3), b"stride_s >= W"),
])
def test_the_launchers_reject_bad_descriptors_before_any_device_call(make, fn, over, text):
    from tecmollm import _lib
    d = make(**over)
    rc = getattr(_lib.lib(), fn)(ctypes.byref(d), None)
    assert rc == -1, (over, rc)                                            # TECM_E_ARG
    assert text in _lib.lib().tecm_last_error(), (over, _lib.lib().tecm_last_error())


def test_the_launchers_reject_a_null_descriptor_and_misaligned_pointers():
    from tecmollm import _lib
    for fn, make, fields in (("tecm_metrics_window", _window_descriptor, ("table", "pred", "err_flag")),
                             ("tecm_block_bootstrap", _boot_descriptor, ("table", "out", "starts"))):
        assert getattr(_lib.lib(), fn)(None, None) == -1 and b"null descriptor" in _lib.lib().tecm_last_error()
        for field in fields:
            d = make()
            setattr(d, field, getattr(d, field) + 2)
            assert getattr(_lib.lib(), fn)(ctypes.byref(d), None) == -2, (fn, field)    # TECM_E_ALIGN
            assert b"aligned" in _lib.lib().tecm_last_error()
    d = _window_descriptor(rows=_buf()[1] + 4)
    assert _lib.lib().tecm_metrics_window(ctypes.byref(d), None) == -2


# ------------------------------------------------------------------------------------ the restated per-window sums
def test_restated_window_sums_add_up_to_the_pooled_statistics():
    """The ordered per-window sums, summed over windows, are the statistics tests/error_maps_ref.py pools -- to rounding:
    both add the same float64 terms, in different orders."""
    from tests import error_maps_ref as ER
    rng = np.random.default_rng(3)
    S, H, I = 4, 3, 135
    pred = (rng.standard_normal((S, H, I)) * 2).astype(np.float32)
    true = (rng.standard_normal((S, H, I)) * 2).astype(np.float32)
    pred[0, 0, 0], pred[1, 1, 1], true[2, 2, 2] = np.nan, np.inf, -np.inf
    table, mags = SR.window_table(pred, true, (21.5, 9.25))
    assert table.shape == mags.shape == (S, H, 8) and (table[:, :, 0] == I).all() and np.isfinite(table).all()
    stats, m2 = np.zeros((1, H, 8, I)), np.zeros((1, H, 8, I))
    ER.accumulate(stats, m2, pred, true, None, (21.5, 9.25))
    assert np.all(np.abs(table.sum(axis=0) - stats[0].sum(axis=2)) <= 1e-12 * mags.sum(axis=0))
    one = SR.window_table(pred[:1, :, :1], true[:1, :, :1])[0]             # one node: the term itself
    t, p = ER.pipeline(pred[:1, :, :1], true[:1, :, :1])
    assert np.array_equal(one[0], ER.terms(t, p)[:, 0, :, 0].T)


# ------------------------------------------------------------------------------------ size of the two methods
@pytest.fixture(scope="module")
def ar1():
    return SR.ar1_columns()                                                # (512, 400), phi = 0.6, seed fixed


def test_dm_size_on_ar1_series(ar1):
    """400 AR(1) series with mean 0 (phi = 0.6, S = 512): the null is true.  At the 5 % level the naive q = 0 test must
    reject far too often (>= 20 %; 33 % expected) and the q = 16 test about as often as it should (<= 12 %)."""
    from tecmollm.significance import dm_statistic
    S, C = ar1.shape
    naive = np.mean([dm_statistic(ar1[:, c], 0)["p"] < 0.05 for c in range(C)])
    hac = np.mean([dm_statistic(ar1[:, c], 16)["p"] < 0.05 for c in range(C)])
    restated = np.mean([SR.dm(ar1[:, c], 16)[1] < 0.05 for c in range(0, C, 8)])
    print(f"rejection at 5 %: q = 0 {naive:.3f}, q = 16 {hac:.3f} (restated on every 8th series {restated:.3f})")
    assert naive >= 0.20
    assert hac <= 0.12
    assert restated == np.mean([dm_statistic(ar1[:, c], 16)["p"] < 0.05 for c in range(0, C, 8)])


def test_block_bootstrap_coverage_on_ar1_series(ar1):
    """The 90 % percentile interval of the mean from R = 300 circular-block replicates (the restated sums; one set of
    starts for all 400 columns): with L = 1 (an iid resample) it covers the true mean 0 far too rarely (<= 70 %), with
    L = 32 about as often as it should ([78 %, 95 %])."""
    from tecmollm.significance import draw_starts
    S, C = ar1.shape
    cover = {}
    for L in (1, 32):
        starts = draw_starts(S, L, 300, seed=11).numpy()
        sums = SR.bootstrap_sums(ar1[None], starts, L)[:, 0, 0]            # (300, 400)
        cover[L] = SR.coverage_of_zero(sums, S)
    print(f"coverage of 0 by the 90 % interval: L = 1 {cover[1]:.3f}, L = 32 {cover[32]:.3f}")
    assert cover[1] <= 0.70
    assert 0.78 <= cover[32] <= 0.95
