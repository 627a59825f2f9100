"""CPU tests of the raw-data stage's host side: the numpy restatement (tests/preprocess_ref.py) against the fixture the
reference's scripts/preprocess.py::main() produced (tests/golden/preprocess.npz, tools/make_golden_preprocess.py), the
mirrors' time features and date split, the header / binding, the workspace arithmetic and the entry points' argument checks
through the C ABI (no device call is reached)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import preprocess_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = ("train", "val", "test")


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "preprocess.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_both_cases_and_crosses_the_calendar_edges(golden):
    assert golden["cases"].tolist() == ["a", "b"] and int(golden["horizon"]) == 12
    assert golden["a_train_tec"].dtype == np.float32 and golden["a_train_tec"].shape == (90, 3, 5)
    assert golden["b_train_tec"].dtype == np.float64 and golden["b_train_tec"].shape[1:] == (2, 3)
    assert golden["a_train_indices"].dtype == np.float64 and golden["a_train_indices"].shape == (90, 5)
    tf = np.concatenate([golden[f"a_{s}_time_features"] for s in SPLITS])
    assert 365 in tf[:, 1] and 0 in tf[:, 1] and 364 in tf[:, 1]            # day 366, 1 January, 31 December of a common year
    feb29 = golden["a_val_time"].astype("datetime64[s]").astype("datetime64[D]") == np.datetime64("2016-02-29")
    assert feb29.any() and (golden["a_val_time_features"][:len(feb29)][feb29[:28]][:, 1] == 59).all()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "preprocess.npz")) < 345_000


@pytest.mark.parametrize("case", ["a", "b"])
def test_the_restatement_reproduces_the_fixture_bit_for_bit(golden, case):
    H = int(golden["horizon"])
    fm, fs = golden[f"{case}_scaler_mean_"], golden[f"{case}_scaler_scale_"]
    ym, ys = float(golden[f"{case}_target_scaler_mean_"][0]), float(golden[f"{case}_target_scaler_scale_"][0])
    for s in SPLITS:
        tec, idx = golden[f"{case}_{s}_tec"], golden[f"{case}_{s}_indices"]
        T = tec.shape[0] - H
        X, Y = golden[f"{case}_{s}_X"], golden[f"{case}_{s}_Y"]
        assert X.shape == (T,) + tec.shape[1:] + (6,) and Y.shape == (T,) + tec.shape[1:] + (H,) and X.dtype == Y.dtype == np.float32
        assert np.array_equal(PR.build_x(tec, idx, fm, fs, T), X), (case, s)
        assert np.array_equal(PR.build_y(tec, ym, ys, H), Y), (case, s)
        tf = PR.time_features(golden[f"{case}_{s}_time"])[:T]
        assert np.array_equal(tf.astype(np.float32), golden[f"{case}_{s}_time_features"]), (case, s)


@pytest.mark.parametrize("case", ["a", "b"])
def test_the_restated_fit_agrees_with_sklearn(golden, case):
    H = int(golden["horizon"])
    tec, idx = golden[f"{case}_train_tec"], golden[f"{case}_train_indices"]
    T, N = tec.shape[0] - H, tec[0].size
    cols = [tec[:T]] + [idx[:T, k:k + 1] for k in range(5)]
    for c, col in enumerate(cols):
        for fit in (PR.fit_ordered, PR.fit_exact):
            count, mean, var = fit(col)[:3]
            assert count * (1 if c == 0 else N) == int(golden[f"{case}_scaler_n_samples_seen_"])
            want = (0, float(golden[f"{case}_scaler_mean_"][c]), float(golden[f"{case}_scaler_var_"][c]), float(np.abs(col).mean()))
            assert PR.close(mean, var, want), (case, c, fit.__name__)
        assert PR.scale_of(var, mean, count) == pytest.approx(float(golden[f"{case}_scaler_scale_"][c]), rel=1e-12)
    for fit in (PR.fit_ordered, PR.fit_exact):                              # the target scaler: the trapezoid weights
        count, mean, var = fit(tec, taps=H)[:3]
        assert count == int(golden[f"{case}_target_scaler_n_samples_seen_"]) == T * N * H
        want = (0, float(golden[f"{case}_target_scaler_mean_"][0]), float(golden[f"{case}_target_scaler_var_"][0]), float(np.abs(tec).mean()))
        assert PR.close(mean, var, want), (case, fit.__name__)


@pytest.mark.parametrize("rows, H", [(13, 12), (30, 12), (25, 24), (90, 12), (14, 1)])
def test_the_trapezoid_weights(rows, H):
    w = PR.weights(rows, H)
    assert w.sum() == (rows - H) * H and w[0] == 0 and w.max() == min(H, rows - H)
    assert np.array_equal(w, PR.weights_by_counting(rows, H))
    assert np.array_equal(PR.weights(rows, 0), np.ones(rows, dtype=np.int64))


def test_the_mirror_extracts_the_fixtures_time_features(golden):
    from src.features.feature_engineering import extract_time_features
    for case in ("a", "b"):
        for s in SPLITS:
            t = golden[f"{case}_{s}_time"].astype("datetime64[s]")
            want = golden[f"{case}_{s}_time_features"]
            got = extract_time_features(t)
            assert got.shape == (len(t), 4) and np.array_equal(got[:len(want)].astype(np.float32), want), (case, s)
            assert np.array_equal(got, PR.time_features(golden[f"{case}_{s}_time"]))
            assert np.array_equal(extract_time_features(t.astype("datetime64[ns]")), got)
            assert got[:, 2].min() == 0                                     # every split starts again at year 0
    t = golden["a_test_time"].astype("datetime64[s]")                       # 2016-12-29 22:00 onwards
    assert extract_time_features(t, start_year=2013)[0, 2] == 3 and extract_time_features(t, start_year=2013)[-1, 2] == 4
    pd = pytest.importorskip("pandas")
    assert np.array_equal(extract_time_features(pd.DatetimeIndex(t)), extract_time_features(t))


def test_split_by_date_boundaries():
    from src.data.data_loader import split_by_date
    t = np.array(["2021-12-31T22:00", "2022-01-01T00:00", "2023-12-31T22:00", "2024-01-01T00:00", "2013-01-01T00:00",
                  "2025-04-30T22:00"], dtype="datetime64[s]")
    data = {"time": t, "tec": np.arange(6 * 2 * 3, dtype=np.float32).reshape(6, 2, 3),
            "space_weather_indices": np.arange(30, dtype=np.float64).reshape(6, 5), "latitude": np.arange(2.0)}
    out = split_by_date(data)
    assert list(out) == ["train", "val", "test"]
    assert out["train"]["time"].tolist() == t[[0, 4]].tolist() and out["val"]["time"].tolist() == t[[1, 2]].tolist()
    assert out["test"]["time"].tolist() == t[[3, 5]].tolist()
    assert np.array_equal(out["val"]["tec"], data["tec"][[1, 2]]) and np.array_equal(out["test"]["space_weather_indices"], data["space_weather_indices"][[3, 5]])
    assert all(out[s]["latitude"] is data["latitude"] for s in out)
    masks = PR.split_masks(t.astype(np.int64))
    assert all(np.array_equal(out[s]["time"], t[masks[s]]) for s in out)


def _struct_names(header, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"[\s*](\w+)\s*[,;]", body)


def test_header_binding_and_build_agree_on_the_new_symbols():
    import tecmollm
    from tecmollm import _lib
    header = open(os.path.join(ROOT, "include", "tecmollm.h")).read()
    for define, value in (("TECM_MOMENTS_MAX_BLOCKS", 2048), ("TECM_FEATURES_MAX_CI", 15)):
        assert f"#define {define} {value}" in header and getattr(_lib, define) == value
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for fn, struct, arg in (("tecm_moments", "TecmMoments", "m"), ("tecm_features_build", "TecmFeaturesBuild", "f"),
                            ("tecm_window_batch_series", "TecmWindowBatchSeries", "w")):
        assert f"int {fn}(const {struct}* {arg}, void* stream);" in header
        assert fn in _lib.EXPORTS and hasattr(handle, fn)
        assert _struct_names(header, struct) == [f[0] for f in getattr(_lib, struct)._fields_], struct
    assert "int64_t tecm_moments_ws_bytes(const TecmMoments* m);" in header and "tecm_moments_ws_bytes" in _lib.EXPORTS
    assert ctypes.sizeof(_lib.TecmMoments) == 8 * 4 + 4 * 4 + 8 * 4
    assert ctypes.sizeof(_lib.TecmFeaturesBuild) == 8 * 2 + 8 * 2 + 4 * 6 + 8 * 2 + 8 * 2 + 8 * 3
    assert ctypes.sizeof(_lib.TecmWindowBatchSeries) == 8 * 5 + 8 * 3 + 4 * 6 + 8 * 3
    assert ctypes.sizeof(_lib.TecmWindowBatch) == 8 * 5 + 8 * 2 + 4 * 6 + 8 * 3       # unchanged
    # each declaration cites the reference lines it replaces
    for cite in ("feature_engineering.py:161-170", "preprocess.py:56-60", "feature_engineering.py:38-67", "preprocess.py:75-83",
                 "src/data/dataset.py:88-93"):
        assert cite in header, cite
    assert _lib.ABI_VERSION == 21 == int(re.search(r"#define\s+TECM_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.lib().tecm_abi_version()
    entry = __import__("__graft_entry__")
    assert "preprocess.hip" in entry.SOURCES
    rules = entry.SPILL_CEILINGS["preprocess.hip"]
    assert sorted(r[0] for r in rules) == sorted(f"{k}_kernel" for k in ("moments_pool", "moments_col", "moments_join", "features_x",
                                                                         "features_ys", "features_y"))
    assert all(r[1:] == ("ScratchSize [bytes/lane]", 0) for r in rules)
    kernels = set(re.findall(r"__global__ __launch_bounds__\(\d+\) void (\w+)\(", open(os.path.join(ROOT, "tec-mollm_amd", "csrc", "preprocess.hip")).read()))
    assert kernels == {r[0] for r in rules}                                  # every kernel of the file has a ceiling
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for fn in ("tecm_moments", "tecm_features_build", "tecm_window_batch_series"):
        assert f"| `{fn}`" in integration, fn
    for name in ("preprocess", "DeviceStandardScaler", "preprocess_splits"):
        assert name in tecmollm.__all__ and getattr(tecmollm, name) is not None


def _buf():
    buf = (ctypes.c_double * 32)()                                         # a real, aligned host address: never dereferenced
    return buf, ctypes.addressof(buf)


def _moments(**over):
    from tecmollm import _lib
    buf, a = _buf()
    f = dict(src=a, rows=20, cols=3, ld=3, src_f64=0, pool=1, taps=0, count=a, mean=a, var=a, ws=a)
    f.update(over)
    d = _lib.TecmMoments(**f)
    d._keep = buf
    return d


def _features(**over):
    from tecmollm import _lib
    buf, a = _buf()
    ones = (ctypes.c_double * 6)(*([1.0] * 6))
    f = dict(tec=a, idx=a, rows=20, x_rows=20, N=3, Ci=5, H=12, tec_f64=0, idx_f64=1, mean=ones, scale=ones, ymean=0.0, yscale=1.0,
             X=a, Ys=a, Y=a)
    f.update(over)
    for k in ("mean", "scale"):
        if isinstance(f[k], (list, tuple)):
            f[k] = (ctypes.c_double * len(f[k]))(*f[k])
    d = _lib.TecmFeaturesBuild(**f)
    d._keep = (buf, ones, f["mean"], f["scale"])
    return d


def _series(**over):
    from tecmollm import _lib
    buf, a = _buf()
    starts = (ctypes.c_int64 * 2)(0, 3)
    f = dict(X=a, TF=a, Ys=a, starts=a, starts_host_check=ctypes.addressof(starts), T=10, Ty=14, row=18, N=3, L_in=7, L_out=4, F_t=4,
             B=2, x_out=a, tf_out=a, y_out=a)
    if "starts_values" in over:
        starts = (ctypes.c_int64 * 2)(*over.pop("starts_values"))
        f["starts_host_check"] = ctypes.addressof(starts)
    f.update(over)
    d = _lib.TecmWindowBatchSeries(**f)
    d._keep = (buf, starts)
    return d


def test_moments_workspace_arithmetic():
    from tecmollm import _lib
    ws = _lib.lib().tecm_moments_ws_bytes
    assert ws(ctypes.byref(_moments(rows=1, cols=1, ld=1))) == 16                    # one block's (sum, count)
    assert ws(ctypes.byref(_moments(rows=20, cols=3))) == 16 * 20                    # pooled: 1 column chunk x min(rows, 2048)
    assert ws(ctypes.byref(_moments(rows=39420, cols=2911, ld=2911))) == 16 * 12 * 170      # 12 chunks x floor(2048 / 12) rows
    assert ws(ctypes.byref(_moments(rows=5, cols=1 << 20, ld=1 << 20))) == 16 * 2048         # 4096 chunks capped at 2048, one row
    assert ws(ctypes.byref(_moments(rows=39420, cols=5, ld=5, pool=0))) == 16 * 5 * 20       # per column: ceil(rows / 2048) blocks
    assert ws(ctypes.byref(_moments(rows=1 << 30, cols=5, ld=5, pool=0))) == 16 * 5 * 256
    for bad in (dict(rows=0), dict(cols=0), dict(ld=2), dict(rows=1 << 30, cols=1 << 11, ld=1 << 11), dict(pool=0, cols=65536, ld=65536)):
        assert ws(ctypes.byref(_moments(**bad))) == -1, bad
    assert ws(None) == -1
    assert max(16 * 12 * 170, 16 * 2048) <= 16 * _lib.TECM_MOMENTS_MAX_BLOCKS


@pytest.mark.parametrize("make, fn, over, text", [
    (_moments, "tecm_moments", dict(src=None), b"null pointer"),
    (_moments, "tecm_moments", dict(mean=None), b"null pointer"),
    (_moments, "tecm_moments", dict(ws=None), b"null pointer"),
    (_moments, "tecm_moments", dict(src_f64=2), b"src_f64 must be 0"),
    (_moments, "tecm_moments", dict(pool=3), b"pool must be 0 or 1"),
    (_moments, "tecm_moments", dict(ld=2), b"bad shape"),
    (_moments, "tecm_moments", dict(rows=0), b"bad shape"),
    (_moments, "tecm_moments", dict(taps=20), b"taps must lie in [0, rows)"),
    (_moments, "tecm_moments", dict(taps=-1), b"taps must lie in [0, rows)"),
    (_features, "tecm_features_build", dict(tec=None), b"null pointer"),
    (_features, "tecm_features_build", dict(X=None, Ys=None, Y=None), b"null pointer"),
    (_features, "tecm_features_build", dict(tec_f64=2), b"must be 0 (float32) or 1 (float64)"),
    (_features, "tecm_features_build", dict(idx_f64=-1), b"must be 0 (float32) or 1 (float64)"),
    (_features, "tecm_features_build", dict(x_rows=21), b"bad shape"),
    (_features, "tecm_features_build", dict(Ci=16), b"Ci outside [0, 15]"),
    (_features, "tecm_features_build", dict(idx=None), b"X needs mean, scale"),
    (_features, "tecm_features_build", dict(scale=[1.0, 1.0, 0.0, 1.0, 1.0, 1.0]), b"scale[2] must be non-zero"),
    (_features, "tecm_features_build", dict(yscale=0.0), b"yscale must be non-zero"),
    (_features, "tecm_features_build", dict(H=20), b"Y needs 0 < H < rows"),
    (_features, "tecm_features_build", dict(H=0), b"Y needs 0 < H < rows"),
    (_series, "tecm_window_batch_series", dict(X=None), b"null pointer"),
    (_series, "tecm_window_batch_series", dict(Ys=None), b"targets need Ys"),
    (_series, "tecm_window_batch_series", dict(L_out=0), b"targets need Ys"),
    (_series, "tecm_window_batch_series", dict(TF=None), b"time features need TF"),
    (_series, "tecm_window_batch_series", dict(starts_values=(0, 4)), b"outside [0, T - L_in]"),
    (_series, "tecm_window_batch_series", dict(starts_values=(-1, 0)), b"outside [0, T - L_in]"),
    (_series, "tecm_window_batch_series", dict(Ty=13), b"last target row lies outside the series"),
])
def test_the_launchers_reject_bad_descriptors_before_any_device_call(make, fn, over, text):
    from tecmollm import _lib
    d = make(**over)
    rc = getattr(_lib.lib(), fn)(ctypes.byref(d), None)
    assert rc == -1, (over, rc)                                            # TECM_E_ARG
    assert text in _lib.lib().tecm_last_error(), (over, _lib.lib().tecm_last_error())


def test_the_launchers_reject_a_null_descriptor_and_misaligned_pointers():
    from tecmollm import _lib
    for fn in ("tecm_moments", "tecm_features_build", "tecm_window_batch_series"):
        assert getattr(_lib.lib(), fn)(None, None) == -1 and b"null descriptor" in _lib.lib().tecm_last_error()
    for make, fn, field in ((_moments, "tecm_moments", "mean"), (_features, "tecm_features_build", "Ys")):
        d = make()
        setattr(d, field, getattr(d, field) + 2)
        assert getattr(_lib.lib(), fn)(ctypes.byref(d), None) == -2, fn    # TECM_E_ALIGN
        assert b"aligned" in _lib.lib().tecm_last_error()


def test_the_scaler_object_on_the_host(tmp_path, golden):
    from src.evaluation.metrics import _scaler_params
    from tecmollm import DeviceStandardScaler
    s = DeviceStandardScaler()._set(np.array([60, 60, 0]), np.array([3.0, 7.25, np.nan]), np.array([4.0, 0.0, np.nan]))
    assert s.scale_.tolist()[:2] == [2.0, 1.0] and np.isnan(s.scale_[2]) and s.n_samples_seen_.tolist() == [60, 60, 0]
    t = DeviceStandardScaler(golden["a_target_scaler_mean_"], golden["a_target_scaler_var_"], golden["a_target_scaler_scale_"],
                             int(golden["a_target_scaler_n_samples_seen_"]))
    assert _scaler_params(t) == (float(t.mean_[0]), float(t.scale_[0]))     # accepted wherever scaler= is taken
    path = t.save(str(tmp_path / "target_scaler"))
    assert path.endswith(".npz")
    u = DeviceStandardScaler.load(path)
    assert np.array_equal(u.mean_, t.mean_) and np.array_equal(u.var_, t.var_) and np.array_equal(u.scale_, t.scale_)
    assert u.n_samples_seen_ == t.n_samples_seen_ == 78 * 15 * 12
    x = golden["a_val_tec"].astype(np.float64).reshape(-1, 1)
    assert np.array_equal(t.inverse_transform(t.transform(x)), (x - t.mean_) / t.scale_ * t.scale_ + t.mean_)
    pytest.importorskip("sklearn")
    sk = t.to_sklearn()
    assert type(sk).__name__ == "StandardScaler" and np.array_equal(sk.transform(x), t.transform(x))
    assert np.array_equal(sk.transform(x.astype(np.float32)), t.transform(x.astype(np.float32)))
    assert np.array_equal(sk.inverse_transform(x), t.inverse_transform(x))
