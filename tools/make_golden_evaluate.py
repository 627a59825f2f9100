"""Golden vectors for the evaluation of a test split (tecmollm/evaluate.py, src/models/baselines.py) from the REFERENCE's
own code.

Run where the reference project is checked out:   python tools/make_golden_evaluate.py REFERENCE_DIR

Imports the reference's `test.py` (`get_baseline_predictions`), `src/models/baselines.py` (`HistoricalAverage`),
`src/evaluation/metrics.py` (`evaluate_horizons`) and `src/data/dataset.py` unmodified from REFERENCE_DIR, feeds seeded
inputs and stores inputs and the functions' outputs only, under tests/golden/evaluate_*.npz.  `test.py` imports the model
(torch_geometric, transformers, peft) and `baselines.py` imports statsmodels; neither is needed by the functions called
here, so those module names are pre-seeded with empty placeholders, as oracle/make_golden_shell.py does for
`src.data.data_loader`.
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
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")

KEYS = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg", "mae_by_horizon", "rmse_by_horizon", "r2_by_horizon",
        "pearson_by_horizon")
# (L_in, L_out, dataset stride) of the get_baseline_predictions cases; grid 3 x 5, C = 6
CASES = [(L_in, L_out, stride) for L_in in (7, 16, 48) for L_out in (4, 12) for stride in (1, 3)]
SPARE = 24                  # window starts per case at stride 1


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


def _sequential_mean(x: np.ndarray) -> np.ndarray:
    """(L, ...) fp32 -> the mean over axis 0 by fp32 adds in ascending order and one fp32 division."""
    acc = x[0].copy()
    for t in range(1, x.shape[0]):
        acc = acc + x[t]
    return acc / np.float32(x.shape[0])


def main():
    if len(sys.argv) < 2 and "TECM_REFERENCE" not in os.environ:
        raise SystemExit("usage: make_golden_evaluate.py REFERENCE_DIR   (or set TECM_REFERENCE)")
    ref = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ["TECM_REFERENCE"])
    sys.path.insert(0, ref)
    _placeholder("src.model.tec_mollm", TEC_MoLLM=None)
    _placeholder("statsmodels.tsa.statespace.sarimax", SARIMAX=None)
    spec = importlib.util.spec_from_file_location("reference_test_script", os.path.join(ref, "test.py"))
    ref_test = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_test)
    from src.data.dataset import SlidingWindowSamplerDataset
    from src.evaluation import metrics as RM
    from src.models import baselines as RB
    logging.disable(logging.CRITICAL)
    import joblib
    from sklearn.preprocessing import StandardScaler
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(11)

    def dataset(td, X, Y, TF, L_in, L_out, stride):
        torch.save({"X": torch.from_numpy(X), "Y": torch.from_numpy(Y), "time_features": torch.from_numpy(TF)},
                   os.path.join(td, "test_set.pt"))
        return SlidingWindowSamplerDataset(td, "test", L_in=L_in, L_out=L_out, stride=stride)

    def time_features(T):
        return np.stack([rng.integers(0, 12, T), rng.integers(0, 366, T), rng.integers(0, 13, T),
                         rng.integers(0, 4, T)], axis=1).astype(np.float32)

    # ------------------------------------------------------------ get_baseline_predictions (test.py:46-71)
    H, W, C = 3, 5, 6
    T_max = max(L_in + L_out for L_in, L_out, _ in CASES) - 1 + SPARE
    # feature-scaled series with a spread of magnitudes and signs, so that the add order matters in the last bits
    X = (rng.standard_normal((T_max, H, W, C)) * np.exp(rng.standard_normal((T_max, H, W, C)))).astype(np.float32)
    store = {"X": X, "cases": np.asarray(CASES, dtype=np.int64)}
    for k, (L_in, L_out, stride) in enumerate(CASES):
        T = L_in + L_out - 1 + SPARE                                        # the case's split is X[:T]
        Y = np.zeros((T, H, W, L_out), dtype=np.float32)
        with tempfile.TemporaryDirectory() as td:
            ds = dataset(td, X[:T], Y, time_features(T), L_in, L_out, stride)
            pred = ref_test.get_baseline_predictions(ds, L_in, L_out)
            assert pred.dtype == np.float32 and pred.shape == (len(ds), H, W, L_out), (pred.dtype, pred.shape)
            for i in range(len(ds)):                                        # the arithmetic the kernel is specified by
                want = _sequential_mean(X[i * stride:i * stride + L_in, :, :, 0])
                assert np.array_equal(pred[i], np.repeat(want[:, :, None], L_out, axis=2)), (k, i)
        store[f"pred_{k}"] = pred
    np.savez_compressed(os.path.join(OUT, "evaluate_window_mean.npz"), **store)

    # ------------------------------------------------------------ HistoricalAverage.fit / predict (baselines.py:13-45)
    T, N = 4380, 35                                                         # one year at 2-hour resolution
    tec = np.maximum(np.round(rng.gamma(2.0, 12.0, size=(T, N)) * 64.0), 1.0) / 64.0      # positive, TECU-like, 1/64 steps
    tec = tec.astype(np.float32)
    hours = (np.datetime64("2014-01-01T00", "h") + 2 * np.arange(T).astype("timedelta64[h]"))
    ha = RB.HistoricalAverage()
    ha.fit(tec, hours)
    when = np.datetime64("2015-03-01T00", "h") + rng.integers(0, 24 * 40, size=64).astype("timedelta64[h]")   # odd hours too
    pred = ha.predict(when, N)
    probe = RB.HistoricalAverage()                                          # the slot rule alone: averages[0, s] = s
    probe.averages = np.arange(12, dtype=np.float64)[None, :]
    slots = probe.predict(when, 1)[:, 0].astype(np.int64)
    np.savez_compressed(os.path.join(OUT, "evaluate_historical_average.npz"), tec=tec,
                        hours=hours.astype(np.int64), averages=ha.averages, when=when.astype(np.int64), predict=pred,
                        when_slots=slots)

    # ------------------------------------------------------------ the baseline scored as test.py:199-217 scores it
    H, W, C, L_in, L_out = 3, 4, 6, 16, 12                                  # 12 nodes: the smallest model configuration
    T = L_in + L_out - 1 + SPARE
    scaler = StandardScaler().fit(rng.gamma(2.0, 12.0, size=(4000, 1)))
    X = rng.standard_normal((T, H, W, C)).astype(np.float32)
    Y = (0.6 * X[:, :, :, 0:1] + 0.8 * rng.standard_normal((T, H, W, L_out))).astype(np.float32)
    TF = time_features(T)
    with tempfile.TemporaryDirectory() as td:
        ds = dataset(td, X, Y, TF, L_in, L_out, 1)
        y_pred = ref_test.get_baseline_predictions(ds, L_in, L_out)
        S = len(ds)
        y_pred = y_pred.transpose(0, 3, 1, 2).reshape(S, L_out, H * W, 1)                  # test.py:204-205
        y_true = np.stack([ds[i]["y"].numpy() for i in range(S)])                        # (S, H, W, L_out)
        y_true = y_true.transpose(0, 3, 1, 2).reshape(S, L_out, H * W, 1)                  # test.py:39
        sp = os.path.join(td, "target_scaler.joblib")
        joblib.dump(scaler, sp)
        out = RM.evaluate_horizons(y_true.copy(), y_pred.copy(), sp)
    np.savez_compressed(os.path.join(OUT, "evaluate_split.npz"), X=X, Y=Y, TF=TF, L_in=L_in, L_out=L_out,
                        mean=np.float64(scaler.mean_[0]), scale=np.float64(scaler.scale_[0]),
                        **{f"out_{k}": np.asarray(out[k], dtype=np.float64) for k in KEYS})
    for f in sorted(os.listdir(OUT)):
        if f.startswith("evaluate_"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
