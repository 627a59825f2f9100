"""The second half of the reference's `test.py` on the device: baseline forecasts for a test split, the comparison of a
trained model with them, and the report.

`test.py:46-71` builds its historical-average baseline by walking the dataset sample by sample through
`sample['x'].numpy()`; `SlidingWindowSamplerDataset` keeps the split in HBM and hands out device views, so here the
baseline of every window is computed where the series lives (`tecm_window_baseline`, one launch for any number of windows)
and `get_baseline_predictions` keeps the reference's signature and returns the reference's bits.  `evaluate_split` scores
the model and the baselines in ONE pass over the batches (`test.py:195-217` makes two passes and collects everything on
the host), `improvement` is `test.py:243-251`, `write_report` is `test.py:260-276` without pandas.

`evaluate_maps` is the same pass one level down: besides the per-horizon dicts it keeps every forecast's statistics per
(group of the window, horizon, node) on the device (`MapMetrics`), for error maps and for scores stratified by storm level
(`window_groups_by_index`) or time of day (`window_groups_by_slot`); `write_maps` writes them out.  The reference has no
counterpart: its numbers pool every node and window.

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
from .devcheck import check_device_errors
from .loop import _batches

KINDS = {"mean": _lib.TECM_BASELINE_MEAN, "last": _lib.TECM_BASELINE_LAST, "periodic": _lib.TECM_BASELINE_PERIODIC}
# result-dict names: "HistoricalAverage" is the reference's (test.py:217); the other two are not in the reference
NAMES = {"mean": "HistoricalAverage", "last": "Persistence", "periodic": "DayAgo"}
MODEL_NAME = "TEC-MoLLM"
SARIMA_NAME = "SARIMA"      # a fitted src.models.baselines.SarimaBaseline given as an element of `baselines=`
LINEAR_NAME = "Linear"      # a fitted src.models.baselines.LinearBaseline, likewise
ANALOG_NAME = "Analog"      # a fitted src.models.baselines.AnalogBaseline, likewise


def baseline_name(kind) -> str:
    """The result-dict name of one element of `baselines=`: a kind string of `KINDS`, a fitted `SarimaBaseline`,
    `LinearBaseline` or `AnalogBaseline`, or a fitted `tecmollm.combine.Combination` (its own `name`)."""
    if isinstance(kind, str):
        if kind in KINDS:
            return NAMES[kind]
    elif _is_combination(kind):
        return kind.name
    else:
        from src.models.baselines import AnalogBaseline, LinearBaseline, SarimaBaseline
        for cls, name in ((SarimaBaseline, SARIMA_NAME), (LinearBaseline, LINEAR_NAME), (AnalogBaseline, ANALOG_NAME)):
            if isinstance(kind, cls):
                if (kind.n_candidates_ if cls is AnalogBaseline else kind.coef_) is None:
                    raise ValueError(f"a {cls.__name__} given as a baseline must be fitted")
                return name
    raise ValueError(f"baselines must come from {sorted(KINDS)}, got {kind!r}")


def baseline_forecast(dataset, indices: Sequence[int], kind) -> torch.Tensor:
    """The (B, L_out, N, 1) forecast of one element of `baselines=` for the windows `indices`."""
    return window_baseline(dataset, indices, kind) if isinstance(kind, str) else kind.forecast_windows(dataset, indices)


def _is_combination(kind) -> bool:
    from .combine import Combination
    return isinstance(kind, Combination)


def baseline_names(baselines, groups=None, num_groups=None, where: str = "this evaluation") -> list:
    """The result-dict names of `baselines=`.  A `Combination` among them must not share its name with another entry, and
    one fitted with more than one group needs the evaluation's `groups` / `num_groups` to match: ValueError otherwise."""
    kinds = list(baselines)
    names = [baseline_name(k) for k in kinds]
    for k, name in zip(kinds, names):
        if _is_combination(k):
            if ([MODEL_NAME] + names).count(name) > 1:
                raise ValueError(f"the name {name!r} of a combination collides with another entry of {[MODEL_NAME] + names}")
            k._check_groups(groups, num_groups, where)
    return names


def batch_forecasts(dataset, chunk, out: torch.Tensor, names, kinds, ids=None) -> list:
    """The forecasts a batch is scored on, [(name, (B, L_out, N, 1) tensor)]: the model's output `out`, then `baselines=` in
    the order given.  Plain members are evaluated first; a `Combination` is then handed the model's output and those of its
    members that are themselves listed, and computes the others for itself alone."""
    preds = [None if _is_combination(k) else baseline_forecast(dataset, chunk, k) for k in kinds]
    if any(p is None for p in preds):
        computed = [(k, p) for k, p in zip(kinds, preds) if p is not None]
        preds = [k.forecast_batch(dataset, chunk, out, ids, computed) if p is None else p for k, p in zip(kinds, preds)]
    return [(MODEL_NAME, out)] + list(zip(names, preds))


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


def _score_pass(model, dataset, edge_index, batch_size, scaler, baselines, edge_weight, order, groups, num_groups,
                per_batch=None, per_forecast=None):
    """The one pass over the batches that `evaluate_split`, `evaluate_maps` and `evaluate_conformal` share: every forecast
    feeds a `HorizonMetrics` of its own and, when `num_groups` is given, a `MapMetrics` too.  `per_batch(ordinal, x, tf, y,
    out, ids)`, when given, sees every batch after its forecasts are scored; `per_forecast(name, pred, y, chunk)`, when
    given, sees every scored forecast with its batch's dataset indices (`score_windows`).
    Returns ({name: HorizonMetrics}, {name: MapMetrics})."""
    from src.evaluation.metrics import HorizonMetrics, MapMetrics
    kinds = list(baselines)
    names = baseline_names(kinds, groups, num_groups, "the evaluation")
    model.eval()
    hms: Dict[str, HorizonMetrics] = {}
    mms: Dict[str, MapMetrics] = {}
    for ordinal, chunk in enumerate(_batches(len(dataset), batch_size, order)):
        x, tf, y = dataset.batch(chunk)
        out = model(x, tf, edge_index, edge_weight)
        if not hms:
            for name in [MODEL_NAME] + names:
                hms[name] = HorizonMetrics(out.shape[1], scaler, device=out.device)
                if num_groups is not None:
                    mms[name] = MapMetrics(out.shape[1], out.shape[2], num_groups, scaler, device=out.device)
        ids = None
        if mms and groups is not None:
            ids = groups[torch.as_tensor(chunk, dtype=torch.int64).to(groups.device, non_blocking=True)]
        forecasts = batch_forecasts(dataset, chunk, out, names, kinds, ids)
        for name, pred in forecasts:
            hms[name].update(pred, y)
            if mms:
                mms[name].update(pred, y, ids)
            if per_forecast is not None:
                per_forecast(name, pred, y, chunk)
        if per_batch is not None:
            per_batch(ordinal, x, tf, y, out, ids)
    return hms, mms


@torch.no_grad()
def evaluate_split(model: torch.nn.Module, dataset, edge_index: torch.Tensor, batch_size: int, scaler=None,
                   baselines: Sequence[str] = ("mean",), edge_weight: Optional[torch.Tensor] = None,
                   order: Optional[Sequence[int]] = None, group=None) -> Dict[str, Dict[str, object]]:
    """`test.py:195-217`: {"TEC-MoLLM": ..., "HistoricalAverage": ..., ["Persistence": ..., "DayAgo": ...]}, each value the
    `evaluate_horizons` dict of that forecast against the split's targets.

    One pass over the batches: the model's output and each baseline's stride-0 view are fed in place to a
    `HorizonMetrics` of their own, with no host synchronisation per batch.  An element of `baselines` is a kind string of
    `window_baseline`, a fitted `src.models.baselines.SarimaBaseline`, whose entry is named "SARIMA" (one
    `tecm_sar_forecast` launch per batch), a fitted `LinearBaseline`, named "Linear" (one `tecm_lin_forecast` launch), a
    fitted `AnalogBaseline`, named "Analog" (one `tecm_analog_search` and one `tecm_analog_forecast` launch per batch), or a
    fitted `tecmollm.combine.Combination`, named by its `name` (one `tecm_combine_apply` launch on the model's output and the
    member forecasts of the batch; one fitted with several groups needs `evaluate_maps`' groups); the same holds for `evaluate_maps` and `evaluate_ensemble`.  `order` and `group` as in `loop.validate`:
    a rank evaluates its shard and every rank returns the metrics of the whole split."""
    hms, _ = _score_pass(model, dataset, edge_index, batch_size, scaler, baselines, edge_weight, order, None, None)
    if not hms:
        raise ValueError("evaluate_split() on an empty dataset")
    return {name: hm.merge_(group).compute() for name, hm in hms.items()}


@torch.no_grad()
def evaluate_maps(model: torch.nn.Module, dataset, edge_index: torch.Tensor, batch_size: int, scaler=None,
                  baselines: Sequence[str] = ("mean",), groups: Optional[torch.Tensor] = None, num_groups: int = 1,
                  edge_weight: Optional[torch.Tensor] = None, order: Optional[Sequence[int]] = None, group=None):
    """`evaluate_split` plus, per forecast, its errors per (group, horizon, node): returns (results, maps) with `results`
    exactly what `evaluate_split` returns and `maps[name]` that forecast's `MapMetrics.compute()` -- (G, H, N) arrays
    of count / mae / rmse / bias / r2_score / pearson_r and the pooled dict of every group.

    `groups` holds one int32 id in [0, num_groups) per DATASET index, on the device (`window_groups_by_index`,
    `window_groups_by_slot`); None puts every window in group 0.  The same single pass as `evaluate_split`; an id outside
    its range is skipped by the kernel and raises here.  `order` and `group` as in `evaluate_split`."""
    if groups is not None and (groups.dtype != torch.int32 or groups.shape != (len(dataset),)):
        raise ValueError(f"groups must be an int32 tensor with one id per dataset index ({len(dataset)})")
    hms, mms = _score_pass(model, dataset, edge_index, batch_size, scaler, baselines, edge_weight, order, groups,
                           int(num_groups))
    if not hms:
        raise ValueError("evaluate_maps() on an empty dataset")
    results = {name: hm.merge_(group).compute() for name, hm in hms.items()}
    maps = {name: mm.merge_(group).compute() for name, mm in mms.items()}
    check_device_errors(next(iter(mms.values())).stats.device)
    return results, maps


def _window_groups(series: torch.Tensor, starts: torch.Tensor, L_in: int, L_out: int, edges, span: str, reduce: str,
                   mean: float = 0.0, scale: float = 1.0) -> torch.Tensor:
    """(T,) series, (S,) int64 window starts -> (S,) int32 bucket of the series reduced over every window's span."""
    if span not in ("input", "target"):
        raise ValueError(f"span must be 'input' or 'target', got {span!r}")
    if reduce not in ("max", "min", "last"):
        raise ValueError(f"reduce must be 'max', 'min' or 'last', got {reduce!r}")
    first, length = (starts, L_in) if span == "input" else (starts + L_in, L_out)
    series = series.to(torch.float64) * scale + mean
    if reduce == "last":
        value = series[first + length - 1]
    else:
        windows = series.unfold(0, length, 1)                              # (T - length + 1, length) view
        value = (windows.max(dim=1).values if reduce == "max" else windows.min(dim=1).values)[first]
    bounds = torch.as_tensor(edges, dtype=torch.float64, device=series.device).reshape(-1)
    if bounds.numel() > 1 and not bool((bounds[1:] >= bounds[:-1]).all()):
        raise ValueError("edges must be ascending")
    return torch.bucketize(value, bounds).to(torch.int32)


def _feature_scale(feature_scaler, channel: int):
    if feature_scaler is None:
        return 0.0, 1.0
    if isinstance(feature_scaler, (tuple, list)):
        return float(feature_scaler[0]), float(feature_scaler[1])
    return float(np.asarray(feature_scaler.mean_).reshape(-1)[channel]), float(np.asarray(feature_scaler.scale_).reshape(-1)[channel])


def window_groups_by_index(dataset, channel: int, edges, span: str = "target", feature_scaler=None,
                           reduce: str = "max") -> torch.Tensor:
    """One int32 group id per dataset index, on the device, from a space-weather index: channels 1-5 of `X` (AE, Dst,
    F10.7, Kp, ap) hold one value per time step, broadcast over the grid (feature_engineering.py:27-36), so the series
    is read at node 0.  It is reduced (`max`, `min` or `last`) over the window's L_in input steps (span "input") or its
    L_out target steps (span "target") and bucketed with `edges` as `torch.bucketize` does: id = number of edges below
    the value, a value equal to an edge falls in the lower group; len(edges) + 1 groups.  `feature_scaler` (a fitted
    StandardScaler over X's channels, or a (mean, scale) pair for this channel) undoes the feature scaling first, so that
    `edges` are in the index's own units: Kp bins, Dst thresholds."""
    T, H, W, Cc = dataset.X.shape
    if not 0 <= int(channel) < Cc:
        raise ValueError(f"channel {channel} outside [0, {Cc})")
    mean, scale = _feature_scale(feature_scaler, int(channel))
    starts = torch.tensor(dataset.sample_indices, dtype=torch.int64).to(dataset.X.device)
    return _window_groups(dataset.X[:, 0, 0, int(channel)], starts, dataset.L_in, dataset.L_out, edges, span, reduce,
                          mean, scale)


def window_groups_by_slot(dataset) -> torch.Tensor:
    """The time-of-day slot, 0..11, of every window's first target step (column 0 of the time features), int32 on the
    device: the grouping of a day / night table."""
    starts = torch.tensor(dataset.sample_indices, dtype=torch.int64).to(dataset.X.device)
    return dataset.time_features[starts + dataset.L_in, 0].to(torch.int32)


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


def check_grid(grid: Sequence[int], num_nodes: int) -> None:
    """Raises ValueError unless the (rows, columns) `grid` holds exactly `num_nodes` nodes."""
    if int(np.prod(grid)) != num_nodes:
        raise ValueError(f"grid {tuple(grid)} does not hold {num_nodes} nodes")


def write_maps(maps: Dict[str, Dict[str, object]], output_dir: str, grid: Optional[Sequence[int]] = None) -> Dict[str, str]:
    """The files of `evaluate_maps`' second result: `error_maps.npz` with one array `<forecast>/<metric>` of shape (G, H, N)
    per forecast and metric -- (G, H, *grid) when `grid`, e.g. (41, 71), is given -- and `evaluation_by_group.csv` with one
    row per forecast and group: the number of (window, node) pairs and the four averages of that group's pooled dict.
    numpy and the standard library only.  Returns the two paths."""
    from src.evaluation.metrics import MAP_KEYS
    os.makedirs(output_dir, exist_ok=True)
    arrays = {}
    for name, m in maps.items():
        for k in MAP_KEYS:
            a = np.asarray(m[k])
            if grid is not None:
                check_grid(grid, a.shape[2])
                a = a.reshape(a.shape[0], a.shape[1], *[int(d) for d in grid])
            arrays[f"{name}/{k}"] = a
    npz_path = os.path.join(output_dir, "error_maps.npz")
    np.savez_compressed(npz_path, **arrays)
    csv_path = os.path.join(output_dir, "evaluation_by_group.csv")
    cols = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg")
    with open(csv_path, "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow(["forecast", "group", "count"] + list(cols))
        for name, m in maps.items():
            count = np.asarray(m["count"])
            for g, pooled in enumerate(m["by_group"]):
                wr.writerow([name, g, int(count[g, 0].sum())] + [repr(float(pooled[k])) for k in cols])
    return {"npz": npz_path, "csv": csv_path}
