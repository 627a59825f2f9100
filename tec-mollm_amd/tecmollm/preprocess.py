"""The raw-data stage on the device: what the reference's `scripts/preprocess.py` does over
`src/features/feature_engineering.py`, from the raw splits `load_and_split_data` returns to trainable tensors and the two
scalers.

  moments()               weighted fp64 count / mean / variance of a strided 2-D device view       (tecm_moments)
  build_features()        X, Ys and (for reference-format files) Y of one split in one call         (tecm_features_build)
  DeviceStandardScaler    a StandardScaler fitted by moments(): the feature scaler (TEC pooled, every index column on its
                          own) or, with `taps`, the target scaler fitted on the series by the trapezoid weights of the
                          targets it would be written into -- no H-fold target tensor
  preprocess_splits()     the whole of preprocess.py::main()
  time_features()         extract_time_features (feature_engineering.py:69-102) in numpy

The target is kept as the target-scaled series Ys (T, H, W): `Y[i, n, h]` of the reference is `Ys[i + 1 + h, n]`, so one
resident series serves every L_out (src/data/dataset.py: SeriesWindowDataset).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import TecmFeaturesBuild, TecmMoments, check, lib, stream_ptr

SPLITS = ("train", "val", "test")
LAYOUTS = ("series", "reference")


# ------------------------------------------------------------------ time features (host)
def time_features(time, start_year: Optional[int] = None) -> np.ndarray:
    """(T) datetimes (numpy datetime64 of any unit, or a pandas DatetimeIndex / Series) -> (T, 4) int64
    [time_of_day_slot, day_of_year, year_index, season_index] as feature_engineering.py:69-102 computes them.  The year
    index is relative to the earliest year OF THE ARRAY PASSED IN, as in the reference (:90-91), so a validation or test
    split starts again at 0; `start_year` replaces that minimum."""
    t = np.asarray(getattr(time, "values", time))
    if not np.issubdtype(t.dtype, np.datetime64):
        t = t.astype("datetime64[s]")
    t = t.reshape(-1)
    years = t.astype("datetime64[Y]")
    days = t.astype("datetime64[D]")
    hour = (t.astype("datetime64[h]") - days.astype("datetime64[h]")).astype(np.int64)
    doy = (days - years.astype("datetime64[D]")).astype(np.int64)                       # dayofyear - 1
    year = years.astype(np.int64) + 1970
    month = t.astype("datetime64[M]").astype(np.int64) % 12 + 1
    if start_year is None:
        start_year = int(year.min()) if year.size else 0
    return np.stack([hour // 2, doy, year - int(start_year), (month % 12 + 3) // 3 - 1], axis=-1).astype(np.int64)


# ------------------------------------------------------------------ device plumbing
def _device_matrix(a, device, name: str) -> torch.Tensor:
    """numpy array or tensor (T, ...) -> (T, prod(...)) float32 / float64 tensor on the device, unit stride along a row."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    t = t.to(device)
    if not t.is_cuda:
        raise _lib.TecmError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if t.dim() < 1 or t.shape[0] == 0:
        raise ValueError(f"{name} needs at least one row")
    t = t.reshape(t.shape[0], -1)
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def moments(x: torch.Tensor, pool: bool, taps: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """count (int64), mean, var (float64) of a 2-D device view with unit column stride (a column slice of a wider matrix is
    read in place): one statistic over everything with `pool`, else one per column; `taps` = H weighs row r by the number of
    horizon-H targets that hold it.  No host synchronisation; the same bits on every call."""
    if x.dim() != 2 or not x.is_cuda or x.dtype not in (torch.float32, torch.float64):
        raise ValueError("moments needs a 2-D float32 / float64 device tensor")
    rows, cols = x.shape
    ld = x.stride(0) if rows > 1 else max(cols, x.stride(0))
    if cols > 1 and x.stride(1) != 1:
        raise ValueError("moments needs unit stride along a row")
    S = 1 if pool else cols
    count = torch.empty(S, device=x.device, dtype=torch.int64)
    mean = torch.empty(S, device=x.device, dtype=torch.float64)
    var = torch.empty(S, device=x.device, dtype=torch.float64)
    m = TecmMoments(src=x.data_ptr(), rows=rows, cols=cols, ld=ld, src_f64=int(x.dtype == torch.float64), pool=int(bool(pool)),
                    taps=int(taps), count=count.data_ptr(), mean=mean.data_ptr(), var=var.data_ptr(), ws=None)
    nbytes = lib().tecm_moments_ws_bytes(C.byref(m))
    if nbytes < 0:
        raise ValueError(f"moments: unsupported shape rows={rows}, cols={cols}, ld={ld}")
    ws = torch.empty(nbytes // 8, device=x.device, dtype=torch.float64)
    m.ws = ws.data_ptr()
    check(lib().tecm_moments(C.byref(m), stream_ptr()), "tecm_moments")
    return count, mean, var


def build_features(tec, indices, feature_scaler, target_scaler, horizon: int = 0, x_rows: Optional[int] = None,
                   outputs: Sequence[str] = ("X", "Ys"), device="cuda") -> Dict[str, torch.Tensor]:
    """One split's tensors from its raw series: tec (T, H, W) or (T, N), indices (T, Ci) or None.  `outputs` picks among
    "X" (x_rows, H, W, 1 + Ci), "Ys" (T, H, W) and "Y" (T - horizon, H, W, horizon); the scalers are objects with `mean_`
    and `scale_` (the feature scaler with 1 + Ci entries) and may be None for an output that does not need them."""
    shape = tuple(tec.shape)
    grid = shape[1:] if len(shape) > 2 else (shape[1],)
    tec2 = _device_matrix(tec, device, "tec").contiguous()
    rows, N = tec2.shape
    idx2 = None if indices is None else _device_matrix(indices, device, "space_weather_indices").contiguous()
    Ci = 0 if idx2 is None else idx2.shape[1]
    if idx2 is not None and idx2.shape[0] != rows:
        raise ValueError(f"tec has {rows} rows, the indices {idx2.shape[0]}")
    x_rows = rows if x_rows is None else int(x_rows)
    f = TecmFeaturesBuild(tec=tec2.data_ptr(), idx=None if idx2 is None else idx2.data_ptr(), rows=rows, x_rows=x_rows, N=N, Ci=Ci,
                          H=int(horizon), tec_f64=int(tec2.dtype == torch.float64),
                          idx_f64=int(idx2 is not None and idx2.dtype == torch.float64))
    out, keep = {}, []
    for name in outputs:
        if name not in ("X", "Ys", "Y"):
            raise ValueError(f"unknown output {name!r}")
    if "X" in outputs:
        mean = np.ascontiguousarray(np.asarray(feature_scaler.mean_, dtype=np.float64).reshape(-1))
        scale = np.ascontiguousarray(np.asarray(feature_scaler.scale_, dtype=np.float64).reshape(-1))
        if mean.size != 1 + Ci or scale.size != 1 + Ci:
            raise ValueError(f"the feature scaler holds {mean.size} features, the split {1 + Ci}")
        keep += [mean, scale]
        f.mean = mean.ctypes.data_as(C.POINTER(C.c_double))
        f.scale = scale.ctypes.data_as(C.POINTER(C.c_double))
        out["X"] = torch.empty((x_rows,) + grid + (1 + Ci,), device=tec2.device, dtype=torch.float32)
        f.X = out["X"].data_ptr()
    if "Ys" in outputs or "Y" in outputs:
        ym = np.asarray(target_scaler.mean_, dtype=np.float64).reshape(-1)
        ys = np.asarray(target_scaler.scale_, dtype=np.float64).reshape(-1)
        if ym.size != 1 or ys.size != 1:
            raise ValueError("the target scaler must be fitted on a single feature")
        f.ymean, f.yscale = float(ym[0]), float(ys[0])
    if "Ys" in outputs:
        out["Ys"] = torch.empty((rows,) + grid, device=tec2.device, dtype=torch.float32)
        f.Ys = out["Ys"].data_ptr()
    if "Y" in outputs:
        if not 0 < int(horizon) < rows:
            raise ValueError(f"Y needs 0 < horizon < rows, got horizon={horizon}, rows={rows}")
        out["Y"] = torch.empty((rows - int(horizon),) + grid + (int(horizon),), device=tec2.device, dtype=torch.float32)
        f.Y = out["Y"].data_ptr()
    check(lib().tecm_features_build(C.byref(f), stream_ptr()), "tecm_features_build")
    del keep
    return out


# ------------------------------------------------------------------ the scaler
def _is_constant_feature(var, mean, n_samples):
    """sklearn.preprocessing._data._is_constant_feature (1.7.2): var <= n eps var + (n mean eps)^2."""
    eps = np.finfo(np.float64).eps
    with np.errstate(invalid="ignore"):
        return var <= n_samples * eps * var + (n_samples * mean * eps) ** 2


class DeviceStandardScaler:
    """A StandardScaler (with_mean, with_std) whose fit runs on the device.  `mean_`, `var_`, `scale_` are numpy float64
    arrays, `n_samples_seen_` an int when every feature saw the same number of samples (else an int64 array), as sklearn
    leaves them; a constant feature gets scale 1 by sklearn's rule.  It can be passed wherever the evaluation code takes
    `scaler=`."""

    def __init__(self, mean=None, var=None, scale=None, n_samples_seen=None):
        self.mean_ = None if mean is None else np.asarray(mean, dtype=np.float64).reshape(-1)
        self.var_ = None if var is None else np.asarray(var, dtype=np.float64).reshape(-1)
        self.scale_ = None if scale is None else np.asarray(scale, dtype=np.float64).reshape(-1)
        self.n_samples_seen_ = n_samples_seen

    def _set(self, count: np.ndarray, mean: np.ndarray, var: np.ndarray) -> "DeviceStandardScaler":
        self.mean_, self.var_ = mean.astype(np.float64), var.astype(np.float64)
        self.n_samples_seen_ = int(count[0]) if np.ptp(count) == 0 else count.astype(np.int64)
        with np.errstate(invalid="ignore"):
            scale = np.sqrt(self.var_)
        scale[_is_constant_feature(self.var_, self.mean_, count.astype(np.float64))] = 1.0
        self.scale_ = scale
        return self

    def fit_series(self, tec, indices=None, taps: int = 0, device="cuda") -> "DeviceStandardScaler":
        """Fit on a raw series: tec (T, ...) pooled into feature 0 and, with `indices` (T, Ci), one feature per index column
        whose count is multiplied by the number of nodes (the reference broadcasts the indices over the grid before it
        fits, feature_engineering.py:27-36, :165-170).  `taps` = H fits on the targets of horizon H (preprocess.py:56-60)."""
        tec2 = _device_matrix(tec, device, "tec")
        parts = [moments(tec2, pool=True, taps=taps)]
        if indices is not None:
            idx2 = _device_matrix(indices, device, "space_weather_indices")
            if idx2.shape[0] != tec2.shape[0]:
                raise ValueError(f"tec has {tec2.shape[0]} rows, the indices {idx2.shape[0]}")
            c, m, v = moments(idx2, pool=False, taps=taps)
            parts.append((c * tec2.shape[1], m, v))
        count, mean, var = (torch.cat([p[i] for p in parts]).cpu().numpy() for i in range(3))     # the one synchronisation
        return self._set(count, mean, var)

    @property
    def n_features_in_(self) -> int:
        return int(self.mean_.size)

    def _float(self, x):
        x = np.asarray(x)
        return np.array(x, dtype=x.dtype if x.dtype in (np.float32, np.float64) else np.float64, copy=True)

    def transform(self, x) -> np.ndarray:
        """sklearn's arithmetic on a host array (..., n_features): X -= mean_; X /= scale_ in the array's float type."""
        X = self._float(x)
        X -= self.mean_
        X /= self.scale_
        return X

    def inverse_transform(self, x) -> np.ndarray:
        X = self._float(x)
        X *= self.scale_
        X += self.mean_
        return X

    def to_sklearn(self):
        from sklearn.preprocessing import StandardScaler
        s = StandardScaler()
        s.mean_, s.var_, s.scale_ = self.mean_.copy(), self.var_.copy(), self.scale_.copy()
        s.n_samples_seen_ = self.n_samples_seen_ if np.isscalar(self.n_samples_seen_) else np.asarray(self.n_samples_seen_).copy()
        s.n_features_in_ = self.n_features_in_
        return s

    def save(self, path: str) -> str:
        if not path.endswith(".npz"):
            path += ".npz"
        np.savez(path, mean_=self.mean_, var_=self.var_, scale_=self.scale_, n_samples_seen_=np.asarray(self.n_samples_seen_, dtype=np.int64))
        return path

    @classmethod
    def load(cls, path: str) -> "DeviceStandardScaler":
        with np.load(path, allow_pickle=False) as z:
            n = z["n_samples_seen_"]
            return cls(z["mean_"], z["var_"], z["scale_"], int(n) if n.ndim == 0 else n.astype(np.int64))


def _dump_scaler(scaler, directory: str, stem: str) -> str:
    """`stem`.joblib holding a real StandardScaler when joblib and sklearn are importable, else `stem`.npz."""
    if not isinstance(scaler, DeviceStandardScaler):
        scaler = DeviceStandardScaler(scaler.mean_, scaler.var_, scaler.scale_, scaler.n_samples_seen_)
    try:
        import joblib
        sk = scaler.to_sklearn()
    except ImportError:
        return scaler.save(os.path.join(directory, stem + ".npz"))
    path = os.path.join(directory, stem + ".joblib")
    joblib.dump(sk, path)
    return path


# ------------------------------------------------------------------ preprocess.py::main()
class PreprocessResult(dict):
    """{split: tensors} with the scalers, layout and horizon as attributes (and the files written, if any)."""
    feature_scaler: DeviceStandardScaler
    target_scaler: DeviceStandardScaler
    layout: str
    horizon: int
    files: Dict[str, str]


def preprocess_splits(splits, horizon: int = 12, output_dir: Optional[str] = None, layout: str = "series", feature_scaler=None,
                      target_scaler=None, device="cuda") -> PreprocessResult:
    """`splits` = {"train" | "val" | "test": {"tec": (T, H, W), "space_weather_indices": (T, Ci), "time": datetimes}} as the
    reference's `load_and_split_data` returns it (numpy arrays or device tensors).  Fits as the reference does unless the
    scalers are passed in -- the feature scaler on the training split's first T - horizon rows (feature_engineering.py:131-
    132, :161-170), the target scaler on the training targets (preprocess.py:56-60) -- then builds every split:
      layout "series"     X (T, H, W, C), Ys (T, H, W), time_features (T, 4), horizon       -> {split}_series.pt
      layout "reference"  X (T - horizon, H, W, C), Y (T - horizon, H, W, horizon), time_features (T - horizon, 4), what the
                          reference writes and SlidingWindowSamplerDataset loads                -> {split}_set.pt
    all float32 on the device.  With `output_dir` the files and both scalers are written there."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {LAYOUTS}, got {layout!r}")
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError("horizon must be at least 1")
    if (feature_scaler is None or target_scaler is None) and "train" not in splits:
        raise ValueError("fitting the scalers needs a 'train' split")
    if feature_scaler is None or target_scaler is None:
        tr = splits["train"]
        T = tr["tec"].shape[0]
        if T <= horizon:
            raise ValueError(f"the training split has {T} rows, horizon = {horizon}")
        tec_tr = _device_matrix(tr["tec"], device, "tec")
        if feature_scaler is None:
            idx_tr = _device_matrix(tr["space_weather_indices"], device, "space_weather_indices")
            feature_scaler = DeviceStandardScaler().fit_series(tec_tr[:T - horizon], idx_tr[:T - horizon], device=device)
        if target_scaler is None:
            target_scaler = DeviceStandardScaler().fit_series(tec_tr, taps=horizon, device=device)
    out = PreprocessResult()
    out.feature_scaler, out.target_scaler, out.layout, out.horizon, out.files = feature_scaler, target_scaler, layout, horizon, {}
    for name, data in splits.items():
        T = data["tec"].shape[0]
        tf = torch.from_numpy(time_features(data["time"])).to(torch.float32)
        if layout == "series":
            t = build_features(data["tec"], data["space_weather_indices"], feature_scaler, target_scaler, outputs=("X", "Ys"),
                               device=device)
            out[name] = {"X": t["X"], "Ys": t["Ys"], "time_features": tf.to(t["X"].device), "horizon": horizon}
        else:
            t = build_features(data["tec"], data["space_weather_indices"], feature_scaler, target_scaler, horizon=horizon,
                               x_rows=T - horizon, outputs=("X", "Y"), device=device)
            out[name] = {"X": t["X"], "Y": t["Y"], "time_features": tf[:T - horizon].to(t["X"].device)}
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        for name, tensors in out.items():
            path = os.path.join(output_dir, f"{name}_series.pt" if layout == "series" else f"{name}_set.pt")
            torch.save({k: v.cpu() if isinstance(v, torch.Tensor) else v for k, v in tensors.items()}, path)
            out.files[name] = path
        out.files["scaler"] = _dump_scaler(feature_scaler, output_dir, "scaler")
        out.files["target_scaler"] = _dump_scaler(target_scaler, output_dir, "target_scaler")
    return out
