"""Device mirror of the reference's `src/features/feature_engineering.py`: same names and argument order, thin layers over
`tecmollm.preprocess`.

The one difference: `create_features_and_targets` and `standardize_features` return float32 DEVICE tensors where the
reference returns float64 numpy arrays.  The standardised values are computed from the raw series in float64 and rounded
once, so they hold the bits the reference's arrays have after its `.float()` (scripts/preprocess.py:86-87).
`extract_time_features` runs on the host in numpy.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

from tecmollm import preprocess as P

IDENTITY = P.DeviceStandardScaler(mean=[0.0], var=[1.0], scale=[1.0], n_samples_seen=0)       # physical units: (v - 0) / 1


def extract_time_features(time_data, start_year: Optional[int] = None) -> np.ndarray:
    """(T) datetimes (`pd.DatetimeIndex` or numpy datetime64) -> (T, 4) [time_of_day_slot, day_of_year, year_index,
    season_index] (feature_engineering.py:69-102).  As in the reference the year index is relative to the earliest year of
    the split passed in, so validation and test splits start again at 0; `start_year=` opts out."""
    return P.time_features(time_data, start_year=start_year)


def create_features_and_targets(file_paths: list, horizon: int = 12) -> dict:
    """{split: {"X": (T - horizon, H, W, 6), "Y": (T - horizon, H, W, horizon), "time_features": (T - horizon, 4)}} in
    physical units (feature_engineering.py:104-144), X and Y as float32 device tensors.  Each split also carries its raw
    "tec" and "space_weather_indices", which `standardize_features` fits and scales from."""
    from src.data.data_loader import load_and_split_data
    data_splits = load_and_split_data(file_paths)
    if not data_splits:
        return {}
    processed = {}
    for name, data in data_splits.items():
        T, Ci = data["tec"].shape[0], data["space_weather_indices"].shape[1]
        ident = P.DeviceStandardScaler(mean=np.zeros(1 + Ci), var=np.ones(1 + Ci), scale=np.ones(1 + Ci), n_samples_seen=0)
        t = P.build_features(data["tec"], data["space_weather_indices"], ident, IDENTITY, horizon=horizon, x_rows=T - horizon,
                             outputs=("X", "Y"))
        processed[name] = {"X": t["X"], "Y": t["Y"], "time_features": extract_time_features(data["time"])[:T - horizon],
                           "tec": data["tec"], "space_weather_indices": data["space_weather_indices"]}
    return processed


def standardize_features(processed_splits: dict, scaler_path: str = "data/processed/scaler.joblib"):
    """(standardized_splits, scaler) as feature_engineering.py:146-194: the scaler fitted on the training X and written to
    `scaler_path` (a `.npz` beside it when joblib or sklearn is missing), every split's X standardised."""
    tr = processed_splits["train"]
    rows = tr["X"].shape[0]
    scaler = P.DeviceStandardScaler().fit_series(P._device_matrix(tr["tec"], "cuda", "tec")[:rows],
                                                 P._device_matrix(tr["space_weather_indices"], "cuda", "space_weather_indices")[:rows])
    directory, stem = os.path.dirname(scaler_path) or ".", os.path.splitext(os.path.basename(scaler_path))[0]
    os.makedirs(directory, exist_ok=True)
    P._dump_scaler(scaler, directory, stem)
    standardized = {}
    for name, data in processed_splits.items():
        t = P.build_features(data["tec"], data["space_weather_indices"], scaler, None, x_rows=data["X"].shape[0], outputs=("X",))
        standardized[name] = {"X": t["X"], "Y": data["Y"]}
    return standardized, scaler
