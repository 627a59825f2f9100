"""Golden vectors for the per-cell evaluation metrics (`MapMetrics`, `derive` in src/evaluation/metrics.py) from the
REFERENCE's own code.

Run where the reference project is checked out:   python tools/make_golden_error_maps.py REFERENCE_DIR

Imports the reference's `src/evaluation/metrics.py` unmodified from REFERENCE_DIR and calls its `evaluate_horizons` once
per node on the (S, H, 1) column of that node: the non-finite guard (:137-143) followed by `evaluate_metrics` (:10-89) on
every (horizon, node) cell.  Stores the inputs and the returned numbers only, as arrays, in tests/golden/error_maps.npz.
Needs scikit-learn, scipy and joblib (generation time only).
"""
from __future__ import annotations

import logging
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
S, H, I = 40, 3, 5
CONSTANT_NODE = 2


def main():
    if len(sys.argv) < 2 and "TECM_REFERENCE" not in os.environ:
        raise SystemExit("usage: make_golden_error_maps.py REFERENCE_DIR   (or set TECM_REFERENCE)")
    ref = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ["TECM_REFERENCE"])
    sys.path.insert(0, ref)
    from src.evaluation import metrics as RM
    logging.disable(logging.CRITICAL)
    import joblib
    from sklearn.preprocessing import StandardScaler
    rng = np.random.default_rng(23)
    scaler = StandardScaler().fit(rng.gamma(2.0, 12.0, size=(4000, 1)))
    mean, scale = float(scaler.mean_[0]), float(scaler.scale_[0])

    y_true = rng.standard_normal((S, H, I)).astype(np.float32)
    y_pred = (0.7 * y_true + 0.5 * rng.standard_normal((S, H, I))).astype(np.float32)
    # a node whose target never changes: a scaled value whose unscaled f32 image averages back to itself exactly, so that
    # the reference's np.std(...) > 0 test (:75) sees a constant series as constant
    for cand in np.arange(0.25, 4.0, 0.015625, dtype=np.float32):
        u = scaler.inverse_transform(np.full((S, 1), cand, dtype=np.float32))
        if u.dtype == np.float32 and np.std(u.ravel()) == 0:
            y_true[:, :, CONSTANT_NODE] = cand
            break
    else:
        raise SystemExit("no constant target value with an exact f32 mean found")
    y_pred[3, 1, 0] = np.nan
    y_pred[17, 2, 3] = np.inf
    y_pred[5, 0, 1] = -9.0                                                  # far below 0 TECU after the inverse transform
    y_pred[6, 0, 1] = 40.0                                                  # far above 200 TECU
    y_pred[21, 2, 4] = 25.0
    unscaled = y_pred[np.isfinite(y_pred)].astype(np.float64) * scale + mean
    assert unscaled.min() < 0 and unscaled.max() > 200

    out = {k: np.zeros((H, I)) for k in ("mae", "rmse", "r2_score", "pearson_r")}
    with tempfile.TemporaryDirectory() as td:
        sp = os.path.join(td, "target_scaler.joblib")
        joblib.dump(scaler, sp)
        for i in range(I):
            res = RM.evaluate_horizons(y_true[:, :, i:i + 1].copy(), y_pred[:, :, i:i + 1].copy(), sp)
            out["mae"][:, i] = res["mae_by_horizon"]
            out["rmse"][:, i] = res["rmse_by_horizon"]
            out["r2_score"][:, i] = res["r2_by_horizon"]
            out["pearson_r"][:, i] = res["pearson_by_horizon"]
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "error_maps.npz")
    np.savez_compressed(path, y_true=y_true, y_pred=y_pred, mean=np.float64(mean), scale=np.float64(scale),
                        constant_node=np.int64(CONSTANT_NODE), **{f"out_{k}": v for k, v in out.items()})
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
