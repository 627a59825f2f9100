"""The raw-data stage restated in numpy, written from the definitions in include/tecmollm.h (8) and the behaviour of the
reference's scripts/preprocess.py: trapezoid weights, an ordered fp64 weighted fit, an exactly rounded fit for the device
tests, the transform, the targets, the time features and the date split.  Shares no code with tecmollm/preprocess.py."""
import math

import numpy as np

BOUND = 1e-12                 # above the 4096 dependent fp64 additions * 2^-53 = 4.6e-13 the kernels' contract allows


def weights(rows: int, taps: int) -> np.ndarray:
    """w_r: the number of (i, h), i < rows - taps, h < taps, with i + 1 + h = r; all ones for taps = 0."""
    if taps == 0:
        return np.ones(rows, dtype=np.int64)
    r = np.arange(rows, dtype=np.int64)
    return np.maximum(0, np.minimum(taps - 1, r - 1) - np.maximum(0, r - rows + taps) + 1)


def weights_by_counting(rows: int, taps: int) -> np.ndarray:
    w = np.zeros(rows, dtype=np.int64)
    for i in range(rows - taps):
        for h in range(taps):
            w[i + 1 + h] += 1
    return w


def fit_ordered(x: np.ndarray, taps: int = 0):
    """(count, mean, var) of one statistic over x (rows, cols): fp64 adds in row-major order, NaN skipped."""
    x = np.asarray(x, dtype=np.float64).reshape(x.shape[0], -1)
    w = weights(x.shape[0], taps)
    ok = ~np.isnan(x)
    wx = np.where(ok, w[:, None] * np.where(ok, x, 0.0), 0.0)
    count = int((ok * w[:, None]).sum())
    mean = float(np.cumsum(wx.reshape(-1))[-1]) / count if count else float("nan")
    d = np.where(ok, x - mean, 0.0)
    var = float(np.cumsum((w[:, None] * (d * d)).reshape(-1))[-1]) / count if count else float("nan")
    return count, mean, var


def fit_exact(x: np.ndarray, taps: int = 0):
    """(count, mean, var, mean of |x|) of one statistic, the mean from an exactly rounded sum (math.fsum over w x with x
    split into two halves whose products with the small integer w are exact), the variance from x - mean, its square and the
    sum in the 64-bit-mantissa long double (relative error 1e-18: exact at the 1e-12 the device is held to)."""
    x = np.asarray(x)
    x = x.reshape(x.shape[0], -1).astype(np.float64)
    w = np.broadcast_to(weights(x.shape[0], taps)[:, None], x.shape)
    ok = ~np.isnan(x) & (w > 0)
    xv, wv = x[ok], w[ok].astype(np.float64)
    count = int(wv.sum())
    if count == 0:
        return 0, float("nan"), float("nan"), float("nan")
    hi = xv.astype(np.float32).astype(np.float64)
    lo = xv - hi
    mean = math.fsum(np.concatenate([wv * hi, wv * lo]).tolist()) / count
    d = xv.astype(np.longdouble) - np.longdouble(mean)
    var = float((wv.astype(np.longdouble) * d * d).sum() / count)
    mean_abs = math.fsum((wv * np.abs(xv)).tolist()) / count
    return count, mean, var, mean_abs


def close(got_mean, got_var, want) -> bool:
    """The accuracy contract: the mean within BOUND of the mean of |x|, the variance within BOUND of itself."""
    _, mean, var, mean_abs = want
    return abs(got_mean - mean) <= BOUND * mean_abs and abs(got_var - var) <= BOUND * var


def is_constant(var, mean, n):
    eps = np.finfo(np.float64).eps
    return var <= n * eps * var + (n * mean * eps) ** 2


def scale_of(var, mean, n):
    return 1.0 if is_constant(var, mean, n) else math.sqrt(var)


def transform(v: np.ndarray, mean: float, scale: float) -> np.ndarray:
    """float32((float64(v) - mean) / scale): one subtraction, one division, one rounding."""
    return ((np.asarray(v).astype(np.float64) - np.float64(mean)) / np.float64(scale)).astype(np.float32)


def build_x(tec, idx, mean, scale, x_rows=None) -> np.ndarray:
    """tec (T, H, W), idx (T, Ci) -> X (x_rows, H, W, 1 + Ci)."""
    T = tec.shape[0] if x_rows is None else x_rows
    X = np.empty(tec[:T].shape + (1 + idx.shape[1],), dtype=np.float32)
    X[..., 0] = transform(tec[:T], mean[0], scale[0])
    for k in range(idx.shape[1]):
        X[..., 1 + k] = transform(idx[:T, k], mean[1 + k], scale[1 + k]).reshape((T,) + (1,) * (tec.ndim - 1))
    return X


def build_ys(tec, ymean, yscale) -> np.ndarray:
    return transform(tec, ymean, yscale)


def build_y(tec, ymean, yscale, H) -> np.ndarray:
    """Y[t, ..., h] = Ys[t + 1 + h]."""
    Ys = build_ys(tec, ymean, yscale)
    T = tec.shape[0] - H
    return np.stack([Ys[1 + h:1 + h + T] for h in range(H)], axis=-1)


def time_features(seconds: np.ndarray, start_year=None) -> np.ndarray:
    """(T) seconds since 1970 -> (T, 4) [hour // 2, day of year - 1, year - first year, season] by the civil calendar."""
    import datetime
    rows = []
    for s in np.asarray(seconds).tolist():
        d = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=int(s))
        rows.append([d.hour // 2, d.timetuple().tm_yday - 1, d.year, (d.month % 12 + 3) // 3 - 1])
    out = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    out[:, 2] -= out[:, 2].min() if start_year is None else start_year
    return out


def split_masks(seconds: np.ndarray):
    t = np.asarray(seconds).astype("datetime64[s]")
    return {"train": t <= np.datetime64("2021-12-31T23:59:59"),
            "val": (t >= np.datetime64("2022-01-01T00:00:00")) & (t <= np.datetime64("2023-12-31T23:59:59")),
            "test": t >= np.datetime64("2024-01-01T00:00:00")}


def fit_exact_quantised(x: np.ndarray, taps: int = 0, q: int = 64):
    """fit_exact for NaN-free data that are whole multiples of 1 / q: the weighted sum is exact in int64 and Python's
    integer division rounds the mean correctly -- for series too long for a list of Python floats."""
    x = np.asarray(x)
    x = x.reshape(x.shape[0], -1).astype(np.float64)
    w = weights(x.shape[0], taps)
    xi = np.rint(x * q).astype(np.int64)
    assert np.array_equal(xi / q, x)
    count = int(w.sum()) * x.shape[1]
    mean = int((xi * w[:, None]).sum()) / (q * count)
    d = x.astype(np.longdouble) - np.longdouble(mean)
    var = float((w[:, None].astype(np.longdouble) * d * d).sum() / count)
    return count, mean, var, float((np.abs(x) * w[:, None]).sum() / count)
