"""Mirror of the reference's `src/data/data_loader.py`: the yearly HDF5 files -> {"train" | "val" | "test": {"tec",
"time", "space_weather_indices", ...}}.  `h5py` is imported when a file is read; the date rule of the split is a function
of its own, `split_by_date`, that works on arrays in memory."""
from __future__ import annotations

from typing import Any, Dict, List

import numpy as np

TRAIN_END = np.datetime64("2021-12-31T23:59:59")          # data_loader.py:156-159
VAL_START = np.datetime64("2022-01-01T00:00:00")
VAL_END = np.datetime64("2023-12-31T23:59:59")
TEST_START = np.datetime64("2024-01-01T00:00:00")
INDEX_NAMES = ("AE_Index", "Dst_Index", "F107_Index", "Kp_Index", "ap_Index")


def split_by_date(data: Dict[str, Any]) -> Dict[str, Dict[str, Any]]:
    """The date rule of `_split_data` (data_loader.py:156-178): train up to 2021-12-31 23:59:59, validation 2022-2023, test
    from 2024-01-01.  "time" and every array with more than one axis are cut along axis 0; anything else (coordinates) is
    passed to every split as it is."""
    t = np.asarray(getattr(data["time"], "values", data["time"])).astype("datetime64[s]")
    masks = {"train": t <= TRAIN_END, "val": (t >= VAL_START) & (t <= VAL_END), "test": t >= TEST_START}
    out = {}
    for name, mask in masks.items():
        out[name] = {k: v[mask] if k == "time" or getattr(v, "ndim", 0) > 1 else v for k, v in data.items()}
    return out


def _load_data_from_hdf5(file_path: str) -> dict:
    import h5py
    with h5py.File(file_path, "r") as f:
        data = {"tec": f["ionosphere/TEC"][:], "time": f["coordinates/datetime_utc"][:]}
        g = f["space_weather_indices"]
        cols = [g[n][:] * (g[n].attrs.get("scale_factor", 1.0) if n == "Kp_Index" else 1.0) for n in INDEX_NAMES]
        data["space_weather_indices"] = np.stack(cols, axis=-1)
        for k in ("latitude", "longitude"):
            if f"coordinates/{k}" in f:
                data[k] = f[f"coordinates/{k}"][:]
    return data


def load_and_split_data(file_paths: List[str]) -> Dict[str, Any]:
    """data_loader.py:180-207: read every file, concatenate along time, decode the time strings, split by date."""
    parts = [_load_data_from_hdf5(p) for p in file_paths]
    if not parts:
        return {}
    agg = {k: np.concatenate([d[k] for d in parts], axis=0) for k in ("tec", "time", "space_weather_indices")}
    agg["time"] = np.char.decode(agg["time"]).astype("datetime64[s]")
    for k in ("latitude", "longitude"):
        if k in parts[0]:
            agg[k] = parts[0][k]
    return split_by_date(agg)
