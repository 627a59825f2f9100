"""The second half of the reference's `test.py` on the device: baseline forecasts for a test split, the comparison of a
trained model with them, and the report.

`test.py:46-71` builds its historical-average baseline by walking the dataset sample by sample through
`sample['x'].numpy()`; `SlidingWindowSamplerDataset` keeps the split in HBM and hands out device views, so here the
baseline of every window is computed where the series lives (`tecm_window_baseline`, one launch for any number of windows)
and `get_baseline_predictions` keeps the reference's signature and returns the reference's bits.  `evaluate_split` scores
the model and the baselines in ONE pass over the batches (`test.py:195-217` makes two passes and collects everything on
the host), `improvement` is `test.py:243-251`, `write_report` is `test.py:260-276` without pandas.

All three baselines take one channel of the FEATURE-scaled `X` as it is and are scored against the TARGET-scaled `Y`, as the
reference's own baseline is (`test.py:59` against `:217`): the comparison a `test.py` user has been looking at stays the same.
"""
from __future__ import annotations

import csv
import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import TecmWindowBaseline, check, lib, stream_ptr
from .loop import _batches

KINDS = {"mean": _lib.TECM_BASELINE_MEAN, "last": _lib.TECM_BASELINE_LAST, "periodic": _lib.TECM_BASELINE_PERIODIC}
# result-dict names: "HistoricalAverage" is the reference's (test.py:217); the other two are not in the reference
NAMES = {"mean": "HistoricalAverage", "last": "Persistence", "periodic": "DayAgo"}
MODEL_NAME = "TEC-MoLLM"


def _launch(dataset, indices: Sequence[int], kind: str, channel: int, period: int, L_out: int, out: torch.Tensor,
            strides) -> None:
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
    if kind == "periodic" and not 0 < period <= dataset.L_in:
        raise ValueError(f"the periodic baseline needs 0 < period <= L_in (period {period}, L_in {dataset.L_in})")
    idx = [int(i) for i in indices]
    for i in idx:
        if not 0 <= i < dataset.num_samples:
            raise IndexError(f"Index {i} is out of bounds for a dataset of size {dataset.num_samples}")
    T, H, W, Cc = dataset.X.shape
    host = torch.tensor([dataset.sample_indices[i] for i in idx], dtype=torch.int64)
    starts = host.to(dataset.X.device, non_blocking=True)
    w = TecmWindowBaseline(X=dataset.X.data_ptr(), starts=starts.data_ptr(), starts_host_check=host.data_ptr(), T=T,
                           N=H * W, C=Cc, channel=int(channel), L_in=dataset.L_in, L_out=int(L_out), B=len(idx),
                           mode=KINDS[kind], period=int(period), out=out.data_ptr(), o_stride_b=strides[0],
                           o_stride_h=strides[1], o_stride_n=strides[2])
    check(lib().tecm_window_baseline(C.byref(w), stream_ptr()), "tecm_window_baseline")


def window_baseline(dataset, indices: Sequence[int], kind: str = "mean", channel: int = 0, period: int = 12) -> torch.Tensor:
    """Baseline forecasts for the windows `indices` of a `SlidingWindowSamplerDataset` as a device tensor of shape
    (B, L_out, N, 1), the layout of the model's output and of `dataset.batch`'s target.

    kind "mean": the average of the input window (the reference's baseline, test.py:57-62, same bits); "last": the
    window's last step (persistence); "periodic": the step `period` before each target step's slot, x[L_in - period +
    (h mod period)] (period 12 at two-hourly resolution: the same hour yesterday).  "mean" and "last" hold one value per
    (window, node) and come back as an expanded view whose horizon stride is 0; nothing of size L_out is stored.
    Every kind reads `channel` of the feature-scaled X as it is (see the module docstring)."""
    B, N = len(indices), dataset.X.shape[1] * dataset.X.shape[2]
    if B == 0:
        raise ValueError("window_baseline() needs at least one window")
    if kind == "periodic":
        out = torch.empty(B, dataset.L_out, N, device=dataset.X.device, dtype=torch.float32)
        _launch(dataset, indices, kind, channel, period, dataset.L_out, out, (dataset.L_out * N, N, 1))
        return out.unsqueeze(-1)
    out = torch.empty(B, N, device=dataset.X.device, dtype=torch.float32)
    _launch(dataset, indices, kind, channel, period, dataset.L_out, out, (N, 0, 1))
    return out.view(B, 1, N, 1).expand(B, dataset.L_out, N, 1)


def get_baseline_predictions(test_dataset, L_in: int, L_out: int) -> np.ndarray:
    """`test.py:46-71` with its signature and its return value: a numpy (num_samples, H, W, L_out) float32 array holding,
    for every sample of the dataset, the time average of channel 0 of its input window repeated over the horizons -- the
    bits the reference's function returns.  As there, the window is the dataset's own (`L_in` is not used) and `L_out`
    only sets how often the average is repeated.  All windows are assembled on the device by one launch and copied to the
    host once.  A `test.py` user swaps the import of this one function and keeps the rest of the script."""
    T, H, W, _ = test_dataset.X.shape
    S, N = len(test_dataset), H * W
    if S == 0:
        return np.zeros((0, H, W, int(L_out)), dtype=np.float32)
    out = torch.empty(S, H, W, int(L_out), device=test_dataset.X.device, dtype=torch.float32)
    _launch(test_dataset, range(S), "mean", 0, 0, int(L_out), out, (N * int(L_out), 1, int(L_out)))
    return out.cpu().numpy()


@torch.no_grad()
def evaluate_split(model: torch.nn.Module, dataset, edge_index: torch.Tensor, batch_size: int, scaler=None,
                   baselines: Sequence[str] = ("mean",), edge_weight: Optional[torch.Tensor] = None,
                   order: Optional[Sequence[int]] = None, group=None) -> Dict[str, Dict[str, object]]:
    """`test.py:195-217`: {"TEC-MoLLM": ..., "HistoricalAverage": ..., ["Persistence": ..., "DayAgo": ...]}, each value the
    `evaluate_horizons` dict of that forecast against the split's targets.

    One pass over the batches: the model's output and each baseline's stride-0 view are fed in place to a
    `HorizonMetrics` of their own, with no host synchronisation per batch.  `order` and `group` as in `loop.validate`:
    a rank evaluates its shard and every rank returns the metrics of the whole split."""
    from src.evaluation.metrics import HorizonMetrics
    kinds = list(baselines)
    for k in kinds:
        if k not in KINDS:
            raise ValueError(f"baselines must come from {sorted(KINDS)}, got {k!r}")
    model.eval()
    hms: Dict[str, HorizonMetrics] = {}
    for chunk in _batches(len(dataset), batch_size, order):
        x, tf, y = dataset.batch(chunk)
        out = model(x, tf, edge_index, edge_weight)
        if not hms:
            for name in [MODEL_NAME] + [NAMES[k] for k in kinds]:
                hms[name] = HorizonMetrics(out.shape[1], scaler, device=out.device)
        hms[MODEL_NAME].update(out, y)
        for k in kinds:
            hms[NAMES[k]].update(window_baseline(dataset, chunk, k), y)
    if not hms:
        raise ValueError("evaluate_split() on an empty dataset")
    return {name: hm.merge_(group).compute() for name, hm in hms.items()}


def improvement(results: Dict[str, Dict[str, object]], model: str = MODEL_NAME,
                baseline: str = "HistoricalAverage") -> Dict[str, float]:
    """The four percentages of `test.py:243-251`: how much lower the model's average MAE and RMSE are than the baseline's,
    and how much higher its average R^2 (relative to |baseline R^2|, which may be negative) and Pearson r."""
    m, b = results[model], results[baseline]
    return {
        "mae": (b["mae_avg"] - m["mae_avg"]) / b["mae_avg"] * 100,
        "rmse": (b["rmse_avg"] - m["rmse_avg"]) / b["rmse_avg"] * 100,
        "r2_score": (m["r2_score_avg"] - b["r2_score_avg"]) / abs(b["r2_score_avg"]) * 100,
        "pearson_r": (m["pearson_r_avg"] - b["pearson_r_avg"]) / b["pearson_r_avg"] * 100,
    }


def _plain(v):
    """numpy scalars / arrays -> Python floats and lists, so that `repr` is the number itself."""
    if isinstance(v, (list, tuple, np.ndarray)):
        return [_plain(x) for x in v]
    return float(v) if isinstance(v, (np.floating, np.integer)) else v


def write_report(results: Dict[str, Dict[str, object]], output_dir: str) -> Dict[str, str]:
    """`test.py:260-276`: `evaluation_results.csv` (one row per model, one column per key of its dict, first header cell
    empty, list-valued cells as their `repr` -- the file `pandas.DataFrame(results).T.to_csv` writes) and
    `evaluation_summary.txt` (per model the four averages to six decimals; the labels are in English here).  Standard
    library only.  Returns the two paths."""
    os.makedirs(output_dir, exist_ok=True)
    keys = []
    for metrics in results.values():
        keys += [k for k in metrics if k not in keys]
    csv_path = os.path.join(output_dir, "evaluation_results.csv")
    with open(csv_path, "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow([""] + keys)
        for name, metrics in results.items():
            wr.writerow([name] + [repr(_plain(metrics[k])) if k in metrics else "" for k in keys])
    txt_path = os.path.join(output_dir, "evaluation_summary.txt")
    with open(txt_path, "w", encoding="utf-8") as f:
        f.write("TEC-MoLLM evaluation summary\n")
        f.write("=" * 50 + "\n\n")
        for name, metrics in results.items():
            f.write(f"{name}:\n")
            f.write(f"  mean MAE:  {metrics['mae_avg']:.6f}\n")
            f.write(f"  mean RMSE: {metrics['rmse_avg']:.6f}\n")
            f.write(f"  mean R2:   {metrics['r2_score_avg']:.6f}\n")
            f.write(f"  mean Pearson R: {metrics['pearson_r_avg']:.6f}\n\n")
    return {"csv": csv_path, "summary": txt_path}
