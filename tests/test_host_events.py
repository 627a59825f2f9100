"""CPU tests of the event-verification feature's host side: `derive_events` against hand tables and the formulas evaluated
directly, the Brier decomposition and the ROC area from hand histograms, `derive_fss`, the restatement's brute-force box sums
against a summed-area table, the threshold constructors, what the two launchers refuse through the C ABI (no device call is
reached), and the header / binding / build entries."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from tests import events_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-12      # a handful of float64 roundings (<= ~10 ulp of values of order 1) lie between two ways of writing a ratio


def _hist_k1(a, b, c, d):
    """(1, 1, 1, 2, 2, 1) counts of one cell with a hits, b false alarms, c misses, d correct negatives."""
    h = np.zeros((1, 1, 1, 2, 2, 1), dtype=np.int64)
    h[0, 0, 0, 1, 0, 0], h[0, 0, 0, 1, 1, 0] = a + b, a
    h[0, 0, 0, 0, 0, 0], h[0, 0, 0, 0, 1, 0] = c + d, c
    return h


def test_derive_events_on_a_table_with_every_class_populated():
    from src.evaluation.metrics import EVENT_CATEGORICAL_KEYS, EVENT_KEYS, derive_events
    a, b, c, d = 28.0, 72.0, 23.0, 2680.0                                  # Finley's tornado table
    n = a + b + c + d
    out = derive_events(_hist_k1(28, 72, 23, 2680))
    assert out["table"].shape == (1, 1, 1, 4, 1) and out["table"][0, 0, 0, :, 0].tolist() == [a, b, c, d]
    assert out["count"][0, 0, 0, 0] == n
    r = (a + b) * (a + c) / n
    want = {"base_rate": (a + c) / n, "pod": a / (a + c), "far": b / (a + b), "pofd": b / (b + d), "csi": a / (a + b + c),
            "ets": (a - r) / (a + b + c - r), "hss": 2 * (a * d - b * c) / ((a + c) * (c + d) + (a + b) * (b + d)),
            "frequency_bias": (a + b) / (a + c)}
    assert set(want) == set(EVENT_CATEGORICAL_KEYS) and set(EVENT_CATEGORICAL_KEYS) < set(EVENT_KEYS)
    for k, v in want.items():
        for suffix, shape in (("", (1, 1, 1, 1)), ("_pooled", (1, 1, 1)), ("_all", (1, 1))):
            got = out[k + suffix]
            assert got.shape == shape and got.dtype == np.float64
            assert abs(float(got.reshape(-1)[0]) - v) <= BAR * abs(v), (k, suffix)
    assert round(want["csi"], 3) == 0.228 and round(want["hss"], 3) == 0.355 and round(want["pod"], 3) == 0.549    # as published
    assert "brier" not in out and "reliability" not in out


def test_derive_events_without_events_and_for_a_perfect_forecast():
    from src.evaluation.metrics import derive_events
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                     # no RuntimeWarning may leak
        none = derive_events(_hist_k1(0, 0, 0, 50))
        empty = derive_events(_hist_k1(0, 0, 0, 0))
        perfect = derive_events(_hist_k1(7, 0, 0, 13))
    for k in ("pod", "far", "csi", "ets", "hss", "frequency_bias"):
        assert np.isnan(none[k]).all() and np.isnan(none[k + "_pooled"]).all() and np.isnan(none[k + "_all"]).all(), k
    assert none["base_rate"][0, 0, 0, 0] == 0.0 and none["pofd"][0, 0, 0, 0] == 0.0
    assert all(np.isnan(empty[k]).all() for k in ("base_rate", "pod", "far", "pofd", "csi", "ets", "hss", "frequency_bias"))
    for k, v in (("pod", 1.0), ("far", 0.0), ("pofd", 0.0), ("csi", 1.0), ("ets", 1.0), ("hss", 1.0), ("frequency_bias", 1.0),
                 ("base_rate", 0.35)):
        assert abs(perfect[k][0, 0, 0, 0] - v) <= BAR, k


def test_pooled_scores_come_from_summed_tables_not_averaged_ratios():
    from src.evaluation.metrics import derive_events
    G, Q, H, N = 2, 3, 4, 5
    rng = np.random.default_rng(0)
    t = rng.integers(0, 40, size=(G, Q, H, 4, N))
    hist = np.zeros((G, Q, H, 2, 2, N), dtype=np.int64)
    hist[:, :, :, 1, 0], hist[:, :, :, 1, 1] = t[:, :, :, 0] + t[:, :, :, 1], t[:, :, :, 0]
    hist[:, :, :, 0, 0], hist[:, :, :, 0, 1] = t[:, :, :, 2] + t[:, :, :, 3], t[:, :, :, 2]
    out = derive_events(hist)
    assert np.array_equal(out["table"], t) and np.array_equal(out["table_pooled"], t.sum(axis=4))
    assert np.array_equal(out["table_all"], t.sum(axis=(2, 4)))
    a, b, c, d = (t[:, :, :, k].sum(axis=3).astype(float) for k in range(4))
    np.testing.assert_allclose(out["csi_pooled"], a / (a + b + c), rtol=BAR, atol=0)
    a, b, c, d = (t[:, :, :, k].sum(axis=(2, 3)).astype(float) for k in range(4))
    np.testing.assert_allclose(out["pod_all"], a / (a + c), rtol=BAR, atol=0)
    assert not np.allclose(out["csi_pooled"], out["csi"].mean(axis=3))
    assert out["pod"].shape == (G, Q, H, N) and out["pod_pooled"].shape == (G, Q, H) and out["pod_all"].shape == (G, Q)
    for bad in (hist.astype(np.float64), hist[0]):
        with pytest.raises(ValueError):
            derive_events(bad)


@pytest.mark.parametrize("K", [2, 5, 16])
def test_brier_from_the_histogram_is_the_mean_over_the_expanded_samples(K):
    from src.evaluation.metrics import EVENT_PROBABILISTIC_KEYS, derive_events
    rng = np.random.default_rng(K)
    S = 400
    p_true = rng.random(S)
    j = rng.binomial(K, p_true)                                            # members that say yes
    o = (rng.random(S) < p_true).astype(np.int64)
    hist = np.zeros((1, 1, 1, K + 1, 2, 1), dtype=np.int64)
    hist[0, 0, 0, :, 0, 0] = np.bincount(j, minlength=K + 1)
    hist[0, 0, 0, :, 1, 0] = np.bincount(j, weights=o, minlength=K + 1).astype(np.int64)
    out = derive_events(hist)
    assert set(EVENT_PROBABILISTIC_KEYS) <= set(out)
    bs = float(out["brier"][0, 0, 0, 0])
    assert abs(bs - np.mean((j / K - o) ** 2)) <= BAR
    rel, res, unc = (float(out["brier_" + k][0, 0, 0, 0]) for k in ("reliability", "resolution", "uncertainty"))
    print(f"K = {K}: BS = {bs!r}, BS - (REL - RES + UNC) = {bs - (rel - res + unc):.3e}")
    assert abs(bs - (rel - res + unc)) <= 1e-15
    obar = o.mean()
    assert abs(unc - obar * (1 - obar)) <= BAR and abs(float(out["brier_skill"][0, 0, 0, 0]) - (1 - bs / unc)) <= BAR
    assert out["reliability"].shape == (1, 1, 1, K + 1, 2) and out["roc_curve"].shape == (1, 1, 1, K + 2, 2)
    n = hist[0, 0, 0, :, 0, 0]
    assert out["reliability"][0, 0, 0, :, 0].tolist() == n.tolist()
    seen = n > 0
    np.testing.assert_allclose(out["reliability"][0, 0, 0, seen, 1], hist[0, 0, 0, seen, 1, 0] / n[seen], rtol=BAR)
    assert out["roc_curve"][0, 0, 0, 0].tolist() == [0.0, 0.0] and out["roc_curve"][0, 0, 0, -1].tolist() == [1.0, 1.0]
    assert 0.5 < float(out["roc_area"][0, 0, 0, 0]) < 1.0                  # an informative forecast
    assert out["brier_pooled"].shape == (1, 1, 1) and out["brier_all"].shape == (1, 1)
    assert out["brier_pooled"][0, 0, 0] == out["brier"][0, 0, 0, 0] == out["brier_all"][0, 0]
    # the categorical table of an ensemble: yes when at least half the members say so
    yes = 2 * j >= K
    assert out["table"][0, 0, 0, :, 0].tolist() == [int((yes & (o == 1)).sum()), int((yes & (o == 0)).sum()),
                                                     int((~yes & (o == 1)).sum()), int((~yes & (o == 0)).sum())]


def test_roc_area_of_a_perfect_a_constant_and_an_inverted_forecast():
    from src.evaluation.metrics import derive_events
    K = 4

    def area(pairs):
        hist = np.zeros((1, 1, 1, K + 1, 2, 1), dtype=np.int64)
        for j, n, o in pairs:
            hist[0, 0, 0, j, :, 0] = n, o
        return float(derive_events(hist)["roc_area"][0, 0, 0, 0])
    assert area([(K, 30, 30), (0, 70, 0)]) == 1.0                          # every event announced by all, no other by any
    assert area([(2, 100, 30)]) == 0.5                                     # always the same probability
    assert area([(0, 30, 30), (K, 70, 0)]) == 0.0                          # inverted
    assert area([(K, 30, 30), (K - 1, 70, 0)]) == 1.0                      # still perfectly separated


def test_derive_fss_on_hand_sums():
    from src.evaluation.metrics import derive_fss
    sums = np.zeros((1, 2, 2, 2, 3), dtype=np.int64)
    sums[0, 0, 0, 0] = 2, 4, 4            # 1 - 2/8
    sums[0, 0, 0, 1] = 0, 9, 9            # 1
    sums[0, 0, 1, 0] = 6, 3, 3            # 0
    sums[0, 0, 1, 1] = 4, 10, 6           # 0.75
    base = np.array([[[0.2, 0.4], [0.0, 0.0]]])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = derive_fss(sums, base)
    assert out["fss"].shape == (1, 2, 2, 2) and out["fss"][0, 0].tolist() == [[0.75, 1.0], [0.0, 0.75]]
    assert np.isnan(out["fss"][0, 1]).all() and np.isnan(out["fss_pooled"][0, 1]).all()
    assert out["fss_pooled"].shape == (1, 2, 2) and out["fss_pooled"][0, 0].tolist() == [1 - 8 / 14, 1 - 4 / 34]
    assert out["fss_uniform"].tolist() == [[[0.6, 0.7], [0.5, 0.5]]]
    assert np.array_equal(ER.fss(sums)[0, 0], out["fss"][0, 0])
    with pytest.raises(ValueError):
        derive_fss(sums[0], base)


@pytest.mark.parametrize("rows, cols", [(1, 1), (1, 7), (5, 27)])
def test_brute_force_box_sums_match_a_summed_area_table(rows, cols):
    rng = np.random.default_rng(rows * 100 + cols)
    for density in (0.0, 0.3, 1.0):
        field = rng.random((rows, cols)) < density
        for n in (1, 3, 5, 9, 2 * max(rows, cols) - 1, 127):
            a, b = ER.box_sums(field, n), ER.box_sums_sat(field, n)
            assert np.array_equal(a, b), (rows, cols, n)
            if n >= 2 * max(rows, cols) - 1:
                assert (a == field.sum()).all()                            # the window covers the grid from every cell
            if n == 1:
                assert np.array_equal(a, field.astype(np.int64))
    one = np.zeros((5, 27), dtype=bool)
    one[0, 0] = True
    assert ER.box_sums(one, 3).sum() == 4 and ER.box_sums(one, 3)[1, 1] == 1   # zero padding: the corner sees 4 cells


def test_threshold_constructors_and_their_files(tmp_path):
    import tecmollm
    from tecmollm.events import EventThresholds
    th = EventThresholds.absolute([15.0, 30.0, 45.0])
    assert (th.Q, th.strides, th.dirs, th.num_slots, th.num_nodes) == (3, (1, 0, 0), [1, 1, 1], 1, None)
    assert th.values.dtype == np.float32 and th.values.shape == (3,) and th.labels == ["> 15 TECU", "> 30 TECU", "> 45 TECU"]
    assert th.at(1, 0, 99) == 30.0
    lo = EventThresholds.absolute([5.0, 40.0], below=[True, False], labels=["low", "high"])
    assert lo.dirs == [-1, 1] and lo.labels == ["low", "high"]
    assert EventThresholds.absolute(7.5, below=True).dirs == [-1]
    N = 6
    clim = np.random.default_rng(0).random((N, 12)) * 40 + 5
    rel = EventThresholds.relative(clim)
    assert (rel.Q, rel.strides, rel.dirs, rel.num_slots, rel.num_nodes) == (2, (12 * N, N, 1), [1, -1], 12, N)
    assert rel.values.shape == (2, 12, N) and rel.values.dtype == np.float32
    assert rel.labels == ["> +30% of climatology", "< -30% of climatology"]
    for q, r in enumerate((0.3, -0.3)):
        for slot in (0, 7, 11):
            for node in (0, 5):
                assert rel.at(q, slot, node) == float(np.float32(clim[node, slot] * (1.0 + r)))
    field = ER.threshold_field(rel.values, rel.strides, 2, np.array([[3, 11]]), 1, 2, N)
    assert field.shape == (2, 1, 2, N) and np.array_equal(field[1, 0, 1], rel.values[1, 11])
    for t in (th, lo, rel):
        back = EventThresholds.load(t.save(str(tmp_path / "thresholds.npz")))
        assert np.array_equal(back.values, t.values) and back.values.dtype == np.float32
        assert (back.strides, back.dirs, back.labels, back.num_slots, back.num_nodes) == \
            (t.strides, t.dirs, t.labels, t.num_slots, t.num_nodes)
    with np.load(str(tmp_path / "thresholds.npz"), allow_pickle=False) as z:
        assert sorted(z.files) == ["dirs", "labels", "num_nodes", "num_slots", "strides", "values"]
    with pytest.raises(ValueError):
        EventThresholds.relative(np.zeros((4, 11)))
    with pytest.raises(ValueError):
        EventThresholds(np.zeros(2, dtype=np.float32), (1, 0, 0), [1, 1, 1], ["a", "b", "c"])
    with pytest.raises(ValueError):
        EventThresholds(np.zeros(2, dtype=np.float32), (1, 0, 0), [1, 0], ["a", "b"])
    assert tecmollm.EventThresholds is EventThresholds


# ------------------------------------------------------------------------------------ header, binding, build
def _struct_names(header, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = re.sub(r"\[\w+\]", "", body)
    return re.findall(r"[\s*](\w+)\s*[,;]", body)


def test_header_binding_and_build_agree_on_the_new_symbols():
    import tecmollm
    from src.evaluation import metrics as M
    from tecmollm import _lib, devcheck, ops
    header = open(os.path.join(ROOT, "include", "tecmollm.h")).read()
    for define, value in (("TECM_BAD_SLOT", 128), ("TECM_EVENT_MAX_Q", 8), ("TECM_EVENT_MAX_W", 8), ("TECM_EVENT_LDS_WORDS", 256)):
        assert f"#define {define} {value}" in header and getattr(_lib, define) == value
    assert devcheck.BAD_SLOT == 128 and devcheck.BAD_SLOT in devcheck._NAMES
    assert "int tecm_event_fss_supported(int32_t rows, int32_t cols);" in header
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for fn, struct in (("tecm_event_hist", "TecmEventHist"), ("tecm_event_fss", "TecmEventFss")):
        assert f"int {fn}(const {struct}* e, void* stream);" in header
        assert fn in _lib.EXPORTS and hasattr(handle, fn)
        assert _struct_names(header, struct) == [f[0] for f in getattr(_lib, struct)._fields_], struct
    assert "tecm_event_fss_supported" in _lib.EXPORTS and hasattr(handle, "tecm_event_fss_supported")
    assert ctypes.sizeof(_lib.TecmEventHist) == 8 * 9 + 8 + 4 + 4 + 8 + 4 + 4 + 8 * 2 + 4 * 4 + 8 * 4 + 8 + 4 * 8 + 8 * 3
    assert ctypes.sizeof(_lib.TecmEventFss) == 8 * 8 + 8 + 4 + 4 + 8 + 4 * 4 + 8 * 2 + 4 * 4 + 8 * 4 + 8 + 4 * 8 + 4 * 8 + 8 * 3
    assert _lib.ABI_VERSION == 21 == int(re.search(r"#define\s+TECM_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.lib().tecm_abi_version()
    entry = __import__("__graft_entry__")
    assert "events.hip" in entry.SOURCES and os.path.exists(os.path.join(entry.CSRC, "events.hip"))
    rules = entry.SPILL_CEILINGS["events.hip"]
    assert sorted(r[0] for r in rules) == ["event_fss_kernel", "event_hist_kernel"]
    assert all(r[1:] == ("ScratchSize [bytes/lane]", 0) for r in rules)
    for name in ("EventThresholds", "target_slots", "evaluate_events", "write_events"):
        assert name in tecmollm.__all__ and callable(getattr(tecmollm, name))
    assert "events" in tecmollm.__all__
    for name in ("EventMetrics", "derive_events", "derive_fss", "EVENT_KEYS"):
        assert hasattr(M, name)
    assert callable(ops.event_hist) and callable(ops.event_fss) and callable(ops.event_fss_ok)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "tecm_event_hist" in integration and "tecm_event_fss" in integration and "evaluate_events" in integration


def test_the_fss_predicate_is_pure_host_arithmetic():
    from tecmollm import _lib
    ok = _lib.lib().tecm_event_fss_supported
    assert ok(41, 71) == 1 and ok(1, 1) == 1 and ok(1, 7) == 1 and ok(5, 27) == 1 and ok(71, 41) == 1
    assert ok(0, 5) == 0 and ok(5, 0) == 0 and ok(-1, 5) == 0
    # 768 B of reduction space + 8 (rows + 1) (cols + 1) B of tables + 2 rows cols B of bits (to a multiple of 8) in 64 KiB
    for rows, cols in ((79, 79), (80, 80), (81, 81), (1, 5000), (1, 6476), (1, 6477), (6476, 1), (200, 31), (200, 32), (1000, 1000)):
        need = 768 + 8 * (rows + 1) * (cols + 1) + ((2 * rows * cols + 7) // 8) * 8
        assert ok(rows, cols) == (1 if need <= 65536 else 0), (rows, cols, need)
    assert ok(80, 80) == 0 and ok(79, 79) == 1


def _buf():
    buf = (ctypes.c_double * 8)()                                          # a real, aligned host address: never dereferenced
    return buf, ctypes.addressof(buf)


def _hist_descriptor(**over):
    from tecmollm import _lib
    buf, a = _buf()
    f = dict(members=a, m_stride_k=0, m_stride_s=1, m_stride_h=1, m_stride_i=1, target=a, t_stride_s=1, t_stride_h=1,
             t_stride_i=1, S=1, H=1, G=1, I=1, K=1, Q=1, mean=0.0, scale=1.0, clip=0, num_slots=1, thr=a, th_stride_q=0,
             th_stride_k=0, th_stride_i=0, slot=None, dir=(ctypes.c_int32 * 8)(1, 1, 1, 1, 1, 1, 1, 1), hist=a, group=None,
             err_flag=a)
    f.update(over)
    d = _lib.TecmEventHist(**f)
    d._keep = buf
    return d


def _fss_descriptor(**over):
    from tecmollm import _lib
    buf, a = _buf()
    f = dict(pred=a, p_stride_s=1, p_stride_h=1, p_stride_i=1, target=a, t_stride_s=1, t_stride_h=1, t_stride_i=1,
             S=1, H=1, G=1, I=6, rows=2, cols=3, Q=1, W=1, mean=0.0, scale=1.0, clip=0, num_slots=1, thr=a, th_stride_q=0,
             th_stride_k=0, th_stride_i=0, slot=None, dir=(ctypes.c_int32 * 8)(1, 1, 1, 1, 1, 1, 1, 1),
             widths=(ctypes.c_int32 * 8)(3, 3, 3, 3, 3, 3, 3, 3), sums=a, group=None, err_flag=a)
    f.update(over)
    d = _lib.TecmEventFss(**f)
    d._keep = buf
    return d


def _widths(*w):
    return (ctypes.c_int32 * 8)(*w)


@pytest.mark.parametrize("make, fn, over, text", [
    (_hist_descriptor, "tecm_event_hist", dict(Q=0), b"Q = 0 outside [1, 8]"),
    (_hist_descriptor, "tecm_event_hist", dict(Q=9), b"Q = 9 outside [1, 8]"),
    (_hist_descriptor, "tecm_event_hist", dict(K=0), b"K = 0 outside [1, 64]"),
    (_hist_descriptor, "tecm_event_hist", dict(K=65), b"K = 65 outside [1, 64]"),
    (_hist_descriptor, "tecm_event_hist", dict(err_flag=None), b"null pointer"),
    (_hist_descriptor, "tecm_event_hist", dict(members=None), b"null pointer"),
    (_hist_descriptor, "tecm_event_hist", dict(thr=None), b"null pointer"),
    (_hist_descriptor, "tecm_event_hist", dict(hist=None), b"null pointer"),
    (_hist_descriptor, "tecm_event_hist", dict(S=0), b"bad shape"),
    (_hist_descriptor, "tecm_event_hist", dict(scale=0.0), b"scale must be non-zero"),
    (_hist_descriptor, "tecm_event_hist", dict(dir=(ctypes.c_int32 * 8)(0)), b"dir[q] must be non-zero"),
    (_hist_descriptor, "tecm_event_hist", dict(num_slots=12), b"1 without a slot tensor"),
    (_hist_descriptor, "tecm_event_hist", dict(num_slots=0), b"num_slots must be >= 1"),
    (_hist_descriptor, "tecm_event_hist", dict(G=65536), b"must be <= 65535"),
    (_fss_descriptor, "tecm_event_fss", dict(Q=0), b"Q = 0 outside [1, 8]"),
    (_fss_descriptor, "tecm_event_fss", dict(Q=9), b"Q = 9 outside [1, 8]"),
    (_fss_descriptor, "tecm_event_fss", dict(W=0), b"W = 0 outside [1, 8]"),
    (_fss_descriptor, "tecm_event_fss", dict(W=9), b"W = 9 outside [1, 8]"),
    (_fss_descriptor, "tecm_event_fss", dict(widths=_widths(4)), b"width 4 must be odd"),
    (_fss_descriptor, "tecm_event_fss", dict(widths=_widths(3, 0), W=2), b"width 0 must be odd"),
    (_fss_descriptor, "tecm_event_fss", dict(widths=_widths(129)), b"width 129 must be odd and in [1, 127]"),
    (_fss_descriptor, "tecm_event_fss", dict(I=7), b"is not rows * cols"),
    (_fss_descriptor, "tecm_event_fss", dict(rows=0, I=0), b"bad shape"),
    (_fss_descriptor, "tecm_event_fss", dict(rows=80, cols=80, I=6400), b"tecm_event_fss_supported"),
    (_fss_descriptor, "tecm_event_fss", dict(err_flag=None), b"null pointer"),
    (_fss_descriptor, "tecm_event_fss", dict(sums=None), b"null pointer"),
    (_fss_descriptor, "tecm_event_fss", dict(scale=0.0), b"scale must be non-zero"),
])
def test_the_launchers_reject_bad_descriptors_before_any_device_call(make, fn, over, text):
    from tecmollm import _lib
    d = make(**over)
    rc = getattr(_lib.lib(), fn)(ctypes.byref(d), None)
    assert rc == -1, (over, rc)                                            # TECM_E_ARG
    assert text in _lib.lib().tecm_last_error(), (over, _lib.lib().tecm_last_error())


def test_the_launchers_reject_a_null_descriptor_and_misaligned_pointers():
    from tecmollm import _lib
    for fn, make, fields in (("tecm_event_hist", _hist_descriptor, ("members", "hist", "thr", "err_flag")),
                             ("tecm_event_fss", _fss_descriptor, ("pred", "sums", "thr", "err_flag"))):
        assert getattr(_lib.lib(), fn)(None, None) == -1 and b"null descriptor" in _lib.lib().tecm_last_error()
        for field in fields:
            d = make()
            setattr(d, field, getattr(d, field) + 2)
            assert getattr(_lib.lib(), fn)(ctypes.byref(d), None) == -2, (fn, field)    # TECM_E_ALIGN
            assert b"aligned" in _lib.lib().tecm_last_error()
    d = _fss_descriptor()
    d.sums += 4
    assert _lib.lib().tecm_event_fss(ctypes.byref(d), None) == -2


# ------------------------------------------------------------------------------------ the restatement alone
def test_the_restatement_fills_every_contingency_class_on_the_gpu_tests_inputs():
    """2.5 N(0, 1) through the scaler (21.5, 9.25) against 15 / 30 / 45 TECU at S * H * I = 2025 values: every class of every
    threshold is populated (the smallest holds 93), so a kernel that never fires cannot pass the GPU comparison."""
    rng = np.random.default_rng(2025)
    S, H, I = 5, 3, 135
    pred = (rng.standard_normal((S, H, I)) * 2.5).astype(np.float32)
    true = (rng.standard_normal((S, H, I)) * 2.5).astype(np.float32)
    hist = np.zeros((1, 3, H, 2, 2, I), dtype=np.int64)
    ties = ER.accumulate_hist(hist, pred[None], true, np.array([15.0, 30.0, 45.0], dtype=np.float32), (1, 0, 0), [1, 1, 1],
                              None, (21.5, 9.25))
    assert ties == 0 and hist[:, :, :, :, 0].sum() == 3 * S * H * I
    classes = np.array([[int(c[0, q].sum()) for c in ER.contingency(hist)] for q in range(3)])
    print("hits / false alarms / misses / correct negatives per threshold:", classes.tolist())
    assert classes.sum(axis=1).tolist() == [S * H * I] * 3 and classes.min() >= 1             # every class non-empty
    # groups, slots and both directions, by hand on three values
    hist = np.zeros((2, 2, 1, 2, 2, 3), dtype=np.int64)
    p = np.array([[[1.0, 5.0, 3.0]], [[9.0, 9.0, 9.0]], [[0.0, 0.0, 0.0]]], dtype=np.float32)
    t = np.array([[[5.0, 5.0, 1.0]], [[9.0, 9.0, 9.0]], [[9.0, 9.0, 9.0]]], dtype=np.float32)
    ties = ER.accumulate_hist(hist, p[None], t, np.array([3.0, 3.0], dtype=np.float32), (1, 0, 0), [1, -1], [1, 5, 0], None)
    assert ties == 2                                                       # the forecast 3 equals both thresholds: no event
    assert hist[:, :, :, :, 0].sum() == 2 * 2 * 3                          # two samples counted, the id 5 nowhere
    a, b, c, d = ER.contingency(hist[0, 0])                                # group 0, "> 3": forecast 0 against 9: three misses
    assert (a.sum(), b.sum(), c[0].tolist(), d.sum()) == (0, 0, [1, 1, 1], 0)
    a, b, c, d = ER.contingency(hist[0, 1])                                # "< 3": three false alarms
    assert (a.sum(), b[0].tolist(), c.sum(), d.sum()) == (0, [1, 1, 1], 0, 0)
    a, b, c, d = ER.contingency(hist[1, 0])                                # group 1, "> 3": forecasts 1, 5, 3 against 5, 5, 1
    assert (a[0].tolist(), b[0].tolist(), c[0].tolist(), d[0].tolist()) == ([0, 1, 0], [0, 0, 0], [1, 0, 0], [0, 0, 1])
    a, b, c, d = ER.contingency(hist[1, 1])                                # "< 3"
    assert (a[0].tolist(), b[0].tolist(), c[0].tolist(), d[0].tolist()) == ([0, 0, 0], [1, 0, 0], [0, 0, 1], [0, 1, 0])
