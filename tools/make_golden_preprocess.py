"""Golden vectors for the raw-data stage (tecmollm/preprocess.py, src/features/feature_engineering.py) from the REFERENCE's
own code.

Run where the reference project is checked out:   python tools/make_golden_preprocess.py REFERENCE_DIR

Imports the reference's `scripts/preprocess.py` unmodified and runs its `main()` in a temporary working directory, once per
case.  `src.data.data_loader` (h5py, thirteen yearly files) is replaced by a placeholder whose `load_and_split_data` returns
seeded splits, as oracle/make_golden_shell.py does.  Only data is stored, in tests/golden/preprocess.npz: the raw inputs,
the three splits' `X`, `Y`, `time_features` as main() saved them, and both scalers' `mean_`, `var_`, `scale_`,
`n_samples_seen_`.

Cases: "a" a 3 x 5 grid of float32 gamma-distributed TEC, "b" a 2 x 3 grid of float64 TEC; the indices are float64 in both.
The splits' start dates make the time features cross 31 December, a 29 February and day 366.
"""
from __future__ import annotations

import importlib
import importlib.util
import logging
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "preprocess.npz")

SPLITS = ("train", "val", "test")
# case -> (grid, TEC dtype, {split: (first time step, rows)}); steps of two hours
CASES = {
    "a": ((3, 5), np.float32, {"train": ("2015-12-28T00", 90), "val": ("2016-02-27T00", 40), "test": ("2016-12-29T22", 40)}),
    "b": ((2, 3), np.float64, {"train": ("2019-12-30T04", 30), "val": ("2020-02-28T12", 20), "test": ("2020-12-30T20", 22)}),
}
HORIZON = 12                                            # fixed in scripts/preprocess.py:34


def _placeholder(name: str, **attrs) -> None:
    parts = name.split(".")
    for i in range(1, len(parts)):                       # parent packages: the real one where it exists
        parent = ".".join(parts[:i])
        try:
            importlib.import_module(parent)
        except ImportError:
            sys.modules[parent] = types.ModuleType(parent)
    sys.modules[name] = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(sys.modules[name], k, v)


def make_splits(rng, grid, dtype, spans):
    import pandas as pd
    H, W = grid
    splits = {}
    for name in SPLITS:
        start, rows = spans[name]
        hours = np.datetime64(start, "h") + 2 * np.arange(rows).astype("timedelta64[h]")
        tec = rng.gamma(2.0, 12.0, size=(rows, H, W)).astype(dtype)               # positive, TECU-like
        idx = np.stack([rng.gamma(1.5, 120.0, rows),                              # AE
                        -rng.gamma(2.0, 15.0, rows) + 10.0,                       # Dst
                        rng.normal(120.0, 30.0, rows),                            # F10.7
                        np.round(rng.uniform(0.0, 9.0, rows) * 3.0) / 3.0,        # Kp in thirds
                        np.round(rng.gamma(1.2, 10.0, rows))], axis=-1)           # ap
        splits[name] = {"tec": tec, "space_weather_indices": idx.astype(np.float64), "time": pd.DatetimeIndex(hours)}
    return splits


def main():
    if len(sys.argv) < 2 and "TECM_REFERENCE" not in os.environ:
        raise SystemExit("usage: make_golden_preprocess.py REFERENCE_DIR   (or set TECM_REFERENCE)")
    ref = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ["TECM_REFERENCE"])
    sys.path.insert(0, ref)
    current = {}
    _placeholder("src.data.data_loader", load_and_split_data=lambda file_paths: current["splits"])
    spec = importlib.util.spec_from_file_location("reference_preprocess_script", os.path.join(ref, "scripts", "preprocess.py"))
    ref_pre = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_pre)
    logging.disable(logging.CRITICAL)
    import joblib
    import torch
    rng = np.random.default_rng(23)
    store = {"horizon": np.int64(HORIZON), "cases": np.asarray(sorted(CASES))}
    cwd = os.getcwd()
    for case in sorted(CASES):
        grid, dtype, spans = CASES[case]
        current["splits"] = make_splits(rng, grid, dtype, spans)
        with tempfile.TemporaryDirectory() as td:
            os.chdir(td)
            try:
                ref_pre.main()
                out = os.path.join(td, "data", "processed")
                for name in SPLITS:
                    raw = current["splits"][name]
                    store[f"{case}_{name}_tec"] = raw["tec"]
                    store[f"{case}_{name}_indices"] = raw["space_weather_indices"]
                    store[f"{case}_{name}_time"] = raw["time"].values.astype("datetime64[s]").astype(np.int64)
                    saved = torch.load(os.path.join(out, f"{name}_set.pt"))
                    for k in ("X", "Y", "time_features"):
                        assert saved[k].dtype == torch.float32
                        store[f"{case}_{name}_{k}"] = saved[k].numpy()
                for stem in ("scaler", "target_scaler"):
                    s = joblib.load(os.path.join(out, f"{stem}.joblib"))
                    for attr in ("mean_", "var_", "scale_"):
                        store[f"{case}_{stem}_{attr}"] = np.asarray(getattr(s, attr), dtype=np.float64)
                    store[f"{case}_{stem}_n_samples_seen_"] = np.asarray(s.n_samples_seen_, dtype=np.int64)
            finally:
                os.chdir(cwd)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **store)
    print(os.path.basename(OUT), os.path.getsize(OUT))


if __name__ == "__main__":
    main()
