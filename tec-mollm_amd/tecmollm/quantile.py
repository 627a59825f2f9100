"""Quantile forecasts: a model trained to emit quantiles, the scores it is judged by, and conformalized quantile regression.

MC dropout (`ensemble_forecast`) pays K forwards for an error bar; a split-conformal interval (`calibrate_conformal`) pays
one, but its half-width is one number per (group, horizon, node) whatever the input says.  In between lies a model that
emits quantiles: one forward, and an interval that widens when the input says it should.

  * The model is the existing `TEC_MoLLM` built with `prediction_horizon = Q * L_out` (`quantile_config`) and trained with
    the pinball loss (`PinballLoss(taus)`, `TrainStep(loss=PinballLoss(taus))`: `tecm_pinball_fwd_bwd_strided`).
  * LAYOUT CONVENTION (include/tecmollm.h (3k)): output channel j = q * L_out + h holds level q of horizon h, so
    `out.view(B, Q, L_out, N)` is the quantile tensor, with no copy.  `QuantileModel` wraps the model: its `forward` returns
    the tau = 0.5 level as a (B, L_out, N, 1) view, so every `evaluate_*`, `calibrate_conformal`, `evaluate_events`, ... runs
    on it unchanged; `.quantiles(...)` returns the (B, Q, L_out, N) view.
  * `evaluate_quantiles` is `evaluate_maps` plus `QuantileMetrics` (src/evaluation/metrics.py, `tecm_quantile_stats`): pinball
    loss and reliability per level, the crossing rate, width / coverage / Winkler score of the central intervals and the
    quantile CRPS, per (group, horizon, node).  Crossing levels are sorted (the rearrangement) before they are scored.
  * `calibrate_cqr` conformalizes one pair of levels (CQR: Romano, Patterson and Candes 2019): the score of a calibration
    window is E = max(z_lo - y, y - z_hi) (`tecm_quantile_scores`, written into the score store `tecm_column_select` reads),
    the offset Qhat its ceil((n + 1)(1 - alpha))-th smallest per (group, horizon, node), and [z_lo - Qhat, z_hi + Qhat]
    covers with probability at least 1 - alpha if calibration and forecast windows are exchangeable.

Not covered: recording the pinball step as a graph (`TrainStep.step_graphed` raises), merging a score store across ranks.
"""
from __future__ import annotations

import copy
import csv
import os
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .conformal import TEC_MAX, TEC_MIN, conformal_ranks
from .devcheck import check_device_errors, error_word
from .evaluate import _score_pass, check_grid
from .functions import quantile_levels, quantile_view
from .loop import _batches


def quantile_config(model_config, taus):
    """A copy of a model configuration (a dict, or any object with a `prediction_horizon` attribute) for the quantile
    model of the levels `taus`: `prediction_horizon` multiplied by Q = len(taus)."""
    Q = len(quantile_levels(taus))
    cfg = copy.deepcopy(model_config)
    if isinstance(cfg, dict):
        cfg["prediction_horizon"] = int(cfg["prediction_horizon"]) * Q
    else:
        cfg.prediction_horizon = int(cfg.prediction_horizon) * Q
    return cfg


class QuantileModel(torch.nn.Module):
    """A `TEC_MoLLM` built with prediction_horizon = Q * L_out, seen as a point forecaster: `forward` returns the
    tau = 0.5 level, a (B, L_out, N, 1) VIEW of the model's output (the levels must contain 0.5), `quantiles` the
    (B, Q, L_out, N) view of all levels."""

    def __init__(self, model: torch.nn.Module, taus, L_out: int):
        super().__init__()
        self.taus = quantile_levels(taus)
        if 0.5 not in self.taus:
            raise ValueError(f"a QuantileModel forecasts its tau = 0.5 level: 0.5 must be among the levels {self.taus}")
        self.L_out = int(L_out)
        if self.L_out < 1:
            raise ValueError(f"L_out must be positive, got {L_out}")
        self.model = model
        self.median_index = self.taus.index(0.5)

    @property
    def Q(self) -> int:
        return len(self.taus)

    def _run(self, x, tf, edge_index, edge_weight=None) -> torch.Tensor:
        out = self.model(x, tf, edge_index, edge_weight)
        if out.dim() != 4 or out.shape[1] != self.Q * self.L_out or out.shape[3] != 1:
            raise ValueError(f"the wrapped model must return (B, {self.Q} * {self.L_out}, N, 1), got {tuple(out.shape)}")
        return out

    def forward(self, x, tf, edge_index, edge_weight=None) -> torch.Tensor:
        out = self._run(x, tf, edge_index, edge_weight)
        m = self.median_index
        return out[:, m * self.L_out:(m + 1) * self.L_out]

    def quantiles(self, x, tf, edge_index, edge_weight=None) -> torch.Tensor:
        return quantile_view(self._run(x, tf, edge_index, edge_weight), self.Q)

    def quantiles_of(self, median: torch.Tensor) -> torch.Tensor:
        """The (B, Q, L_out, N) view of all levels behind a tensor that `forward` returned: the median is a slice of the
        model's whole output, so the other levels lie at known offsets around it in the same storage.  No state is kept."""
        if median.dim() != 4 or median.shape[1] != self.L_out or median.shape[3] != 1:
            raise ValueError(f"expected a (B, {self.L_out}, N, 1) result of forward(), got {tuple(median.shape)}")
        sb, sj, sn, s1 = median.stride()
        first = median.storage_offset() - self.median_index * self.L_out * sj
        B, _, N, _ = median.shape
        shape = (B, self.Q * self.L_out, N, 1)
        last = first + sum(st * (sz - 1) for st, sz in zip((sb, sj, sn, s1), shape))
        if first < 0 or min(sb, sj, sn) < 0 or last >= median.untyped_storage().nbytes() // median.element_size():
            raise ValueError("the tensor is not the tau = 0.5 slice of a whole quantile output")
        return quantile_view(median.detach().as_strided(shape, (sb, sj, sn, s1), first), self.Q)


class CQRIntervals:
    """The calibrated offsets of one pair of levels: `offset` (G, L_out, N) float32 numpy in TECU (scaled units without a
    scaler), `pair` = (tau_lo, tau_hi), `alpha` = tau_lo + 1 - tau_hi, `taus` (all levels of the model), `counts` (G)
    calibration windows per group and the target scaler's `mean` / `scale` / `clip`.  A sample's interval is
    [z_lo - offset, z_hi + offset] with z the sorted levels in physical units."""

    def __init__(self, offset, pair, taus, counts, mean: float = 0.0, scale: float = 1.0, clip: bool = False):
        self.offset = np.ascontiguousarray(offset, dtype=np.float32)
        if self.offset.ndim != 3:
            raise ValueError(f"offset must be (G, H, N), got {self.offset.shape}")
        self.taus = quantile_levels(taus)
        self.pair = (float(pair[0]), float(pair[1]))
        if self.pair[0] not in self.taus or self.pair[1] not in self.taus or not self.pair[0] < self.pair[1]:
            raise ValueError(f"pair must name two of the levels {self.taus}, lower first, got {pair}")
        self.lo_idx, self.hi_idx = self.taus.index(self.pair[0]), self.taus.index(self.pair[1])
        self.counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        if self.counts.shape[0] != self.offset.shape[0]:
            raise ValueError("counts must hold one number per group")
        self.mean, self.scale, self.clip = float(mean), float(scale), bool(clip)
        self._device: Dict[str, torch.Tensor] = {}

    @property
    def alpha(self) -> float:
        return float(pair_alpha(self.pair))

    @property
    def num_groups(self) -> int:
        return self.offset.shape[0]

    @property
    def scaler(self) -> Optional[Tuple[float, float]]:
        return (self.mean, self.scale) if self.clip else None

    @property
    def finite(self) -> bool:
        """Whether every group had enough calibration windows for a finite offset at this alpha."""
        return bool(np.isfinite(self.offset).all())

    def on(self, device) -> torch.Tensor:
        """The `adjust` tensor of `QuantileMetrics.update`: (G, H, Q, N) float32 on `device`, -offset at the lower level of
        the pair, +offset at the upper, 0 elsewhere."""
        key = str(torch.device(device))
        if key not in self._device:
            G, H, N = self.offset.shape
            adj = np.zeros((G, H, len(self.taus), N), dtype=np.float32)
            adj[:, :, self.lo_idx] = -self.offset
            adj[:, :, self.hi_idx] = self.offset
            self._device[key] = torch.from_numpy(adj).to(device)
        return self._device[key]

    def save(self, path: str) -> str:
        """One `.npz` of numpy arrays only (loads without pickle)."""
        np.savez(path, offset=self.offset, pair=np.asarray(self.pair, dtype=np.float64),
                 taus=np.asarray(self.taus, dtype=np.float64), counts=self.counts, mean=np.float64(self.mean),
                 scale=np.float64(self.scale), clip=np.asarray(self.clip))
        return path if path.endswith(".npz") else path + ".npz"

    @classmethod
    def load(cls, path: str) -> "CQRIntervals":
        with np.load(path, allow_pickle=False) as z:
            return cls(z["offset"], z["pair"].tolist(), z["taus"].tolist(), z["counts"], float(z["mean"]), float(z["scale"]),
                       bool(z["clip"]))


def pair_alpha(pair) -> Fraction:
    """alpha = tau_lo + 1 - tau_hi of a pair of levels, exact on the decimals as written (`conformal_ranks` takes it)."""
    lo, hi = (Fraction(str(float(t))) for t in pair)
    a = lo + 1 - hi
    if not 0 < a < 1:
        raise ValueError(f"a pair needs tau_lo < tau_hi inside (0, 1), got {tuple(pair)}")
    return a


def _scaler_clip(scaler):
    from src.evaluation.metrics import _scaler_params
    sc = _scaler_params(scaler)
    mean, scale = sc if sc is not None else (0.0, 1.0)
    return sc, mean, scale, (TEC_MIN, TEC_MAX) if sc is not None else None


def _check_groups(groups, dataset) -> None:
    if groups is not None and (groups.dtype != torch.int32 or groups.shape != (len(dataset),)):
        raise ValueError(f"groups must be an int32 tensor with one id per dataset index ({len(dataset)})")


@torch.no_grad()
def calibrate_cqr(qmodel: QuantileModel, val_dataset, edge_index: torch.Tensor, batch_size: int, pair=(0.1, 0.9), scaler=None,
                  groups: Optional[torch.Tensor] = None, num_groups: int = 1, order: Optional[Sequence[int]] = None,
                  edge_weight: Optional[torch.Tensor] = None) -> CQRIntervals:
    """One `eval()` no-grad pass over a calibration split (the `val` split: neither the training split nor the one to be
    scored): the CQR scores of the pair (tau_lo, tau_hi) go into a score store on the device (`tecm_quantile_scores`) and
    `tecm_column_select` takes, per (group, horizon, node), the score of rank `conformal_ranks(n, alpha, "absolute")` with
    alpha = tau_lo + 1 - tau_hi.  `groups`, `num_groups`, `order` as in `calibrate_conformal`; a group with too few windows
    gets +inf (`CQRIntervals.finite`).  One device, one pass."""
    _check_groups(groups, val_dataset)
    pair = (float(pair[0]), float(pair[1]))
    if pair[0] not in qmodel.taus or pair[1] not in qmodel.taus:
        raise ValueError(f"pair must name two of the model's levels {qmodel.taus}, got {pair}")
    alpha = pair_alpha(pair)
    lo_idx, hi_idx = qmodel.taus.index(pair[0]), qmodel.taus.index(pair[1])
    total = len(val_dataset) if order is None else len(list(order))
    if total == 0:
        raise ValueError("calibrate_cqr() on an empty dataset")
    sc, mean, scale, clip = _scaler_clip(scaler)
    G = int(num_groups)
    was_training = qmodel.training
    qmodel.eval()
    store = ids_all = None
    rows = 0
    try:
        for chunk in _batches(len(val_dataset), batch_size, order):
            x, tf, y = val_dataset.batch(chunk)
            lv = qmodel.quantiles(x, tf, edge_index, edge_weight)                 # (B, Q, H, N)
            B, Q, H, N = lv.shape
            if store is None:
                store = torch.empty(total, H * N, device=lv.device, dtype=torch.float32)
                ids_all = torch.zeros(total, device=lv.device, dtype=torch.int32)
            if groups is not None:
                ids_all[rows:rows + B].copy_(groups[torch.as_tensor(chunk, dtype=torch.int64).to(groups.device, non_blocking=True)])
            ops.quantile_scores(lv.permute(1, 0, 2, 3), y[..., 0] if y.dim() == 4 else y, store, rows,
                                lo_idx, hi_idx, mean=mean, scale=scale, clip=clip)
            rows += B
    finally:
        qmodel.train(was_training)
    ids = ids_all[:rows]
    inside = (ids >= 0) & (ids < G)
    counts = torch.bincount(ids[inside].to(torch.int64), minlength=G).cpu().numpy()       # the host sync
    ranks = np.array([[conformal_ranks(int(n), alpha, "absolute")[0]] for n in counts], dtype=np.int32)
    errs = error_word(store.device)
    out = ops.column_select(store[:rows], torch.from_numpy(ranks).to(store.device), ids, errs.ptr())     # (1, G, H*N)
    errs.post()
    check_device_errors(store.device)
    return CQRIntervals(out.cpu().numpy().reshape(G, H, N), pair, qmodel.taus, counts, mean, scale, sc is not None)


def _intervals_fit(intervals: Optional[CQRIntervals], qmodel: QuantileModel, num_groups: int) -> None:
    if intervals is None:
        return
    if intervals.taus != qmodel.taus:
        raise ValueError(f"intervals of the levels {intervals.taus} do not fit a model of {qmodel.taus}")
    if intervals.num_groups not in (1, int(num_groups)):
        raise ValueError(f"intervals of {intervals.num_groups} groups do not fit num_groups = {num_groups}")


@torch.no_grad()
def quantile_forecast(qmodel: QuantileModel, x: torch.Tensor, tf: torch.Tensor, edge_index: torch.Tensor, scaler=None,
                      intervals: Optional[CQRIntervals] = None, groups: Optional[torch.Tensor] = None,
                      edge_weight: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """One `eval()` forward: {"quantiles": (B, Q, L_out, N) sorted levels, "median": (B, L_out, N)}, device tensors in
    TECU (scaled units without a scaler); with a `CQRIntervals` (whose scaler then holds) the pair's levels carry their
    offsets and "lo" / "hi" (B, L_out, N) name the calibrated interval.  `groups` (B) int32 on the device picks every
    sample's group for group-conditional intervals (None: group 0)."""
    G = intervals.num_groups if intervals is not None else 1
    _intervals_fit(intervals, qmodel, G)
    was_training = qmodel.training
    qmodel.eval()
    try:
        lv = qmodel.quantiles(x, tf, edge_index, edge_weight)
    finally:
        qmodel.train(was_training)
    _, mean, scale, clip = _scaler_clip(intervals.scaler if intervals is not None else scaler)
    if groups is not None and (groups.dtype != torch.int32 or groups.shape != (lv.shape[0],)):
        raise ValueError(f"groups must be an int32 tensor with one id per sample ({lv.shape[0]})")
    z = torch.empty(lv.shape, device=lv.device, dtype=torch.float32)
    errs = error_word(lv.device)
    ops.quantile_stats(lv.permute(1, 0, 2, 3), None, qmodel.taus, None, None, mean=mean, scale=scale, clip=clip,
                       adjust=intervals.on(lv.device) if intervals is not None else None,
                       groups=groups.contiguous() if groups is not None else None, num_groups=G, err_flag=errs.ptr(),
                       out_z=z.permute(1, 0, 2, 3))
    if groups is not None:
        errs.post()
        check_device_errors(lv.device)
    got = {"quantiles": z, "median": z[:, qmodel.median_index]}
    if intervals is not None:
        got["lo"], got["hi"] = z[:, intervals.lo_idx], z[:, intervals.hi_idx]
    return got


@torch.no_grad()
def evaluate_quantiles(qmodel: QuantileModel, dataset, edge_index: torch.Tensor, batch_size: int, scaler=None,
                       baselines: Sequence[str] = ("mean",), groups: Optional[torch.Tensor] = None, num_groups: int = 1,
                       intervals: Optional[CQRIntervals] = None, order: Optional[Sequence[int]] = None, group=None,
                       edge_weight: Optional[torch.Tensor] = None):
    """`evaluate_maps` plus the quantile scores: returns (results, maps, quant).  The same single pass (`_score_pass`), so
    `results` and `maps` are what `evaluate_maps(qmodel, ...)` gives bit for bit (the tau = 0.5 level is the forecast); per
    batch all levels of that same forward are scored too (`QuantileMetrics`, whose `compute()` is `quant`).  With
    `intervals` the pair's levels carry their calibrated offsets (and `scaler` must be the one they were calibrated with).
    `groups` / `num_groups`, `order` and `group` as in `evaluate_maps`: the statistics are sums and merge across ranks."""
    from src.evaluation.metrics import QuantileMetrics
    _check_groups(groups, dataset)
    _intervals_fit(intervals, qmodel, num_groups)
    box: List[QuantileMetrics] = []

    def per_batch(ordinal, x, tf, y, out, ids):
        lv = qmodel.quantiles_of(out)                  # `out` is the median slice of the whole output of this forward
        if not box:
            box.append(QuantileMetrics(lv.shape[2], lv.shape[3], qmodel.taus, int(num_groups), scaler, device=lv.device))
        box[0].update(lv, y, ids, intervals.on(lv.device) if intervals is not None else None)

    hms, mms = _score_pass(qmodel, dataset, edge_index, batch_size, scaler, baselines, edge_weight, order, groups,
                           int(num_groups), per_batch)
    if not hms:
        raise ValueError("evaluate_quantiles() on an empty dataset")
    results = {name: hm.merge_(group).compute() for name, hm in hms.items()}
    maps = {name: mm.merge_(group).compute() for name, mm in mms.items()}
    quant = box[0].merge_(group).compute()
    check_device_errors(box[0].stats.device)
    return results, maps, quant


def _tag(tau: float) -> str:
    return f"{tau:g}"


def quantile_csv_columns(taus) -> List[str]:
    """The columns of `quantile_by_horizon.csv` after group and horizon."""
    from src.evaluation.metrics import quantile_pairs
    cols = ["count", "crossing_rate", "quantile_crps"]
    cols += [f"pinball_{_tag(t)}" for t in taus] + [f"reliability_{_tag(t)}" for t in taus]
    for k in ("interval_width", "coverage", "interval_score"):
        cols += [f"{k}_{_tag(lo)}_{_tag(hi)}" for lo, hi, _ in quantile_pairs(taus)]
    return cols


def write_quantiles(quant: Dict[str, object], output_dir: str, grid: Optional[Sequence[int]] = None) -> Dict[str, str]:
    """The files of `evaluate_quantiles`' third result: `quantile_maps.npz` with one array per key of `QUANTILE_KEYS` --
    (G, H, N) and a trailing axis of Q or P where the key has one; (G, H, *grid, ...) when `grid`, e.g. (41, 71), is given --
    plus `taus` and `pairs`; and `quantile_by_horizon.csv` with one row per group and horizon: that group's statistics
    pooled over the nodes (`quantile_csv_columns`).  numpy and the standard library only.  Returns the two paths."""
    from src.evaluation.metrics import QUANTILE_KEYS, QUANTILE_LEVEL_KEYS, QUANTILE_PAIR_KEYS
    os.makedirs(output_dir, exist_ok=True)
    taus = [float(t) for t in quant["taus"]]
    arrays = {}
    for k in QUANTILE_KEYS:
        a = np.asarray(quant[k])
        if grid is not None:
            check_grid(grid, a.shape[2])
            a = a.reshape(a.shape[0], a.shape[1], *[int(d) for d in grid], *a.shape[3:])
        arrays[k] = a
    arrays["taus"] = np.asarray(taus, dtype=np.float64)
    arrays["pairs"] = np.asarray(quant["pairs"], dtype=np.float64).reshape(-1, 3)
    npz_path = os.path.join(output_dir, "quantile_maps.npz")
    np.savez_compressed(npz_path, **arrays)
    csv_path = os.path.join(output_dir, "quantile_by_horizon.csv")
    with open(csv_path, "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow(["group", "horizon"] + quantile_csv_columns(taus))
        for g, pooled in enumerate(quant["by_group"]):
            for h in range(len(pooled["count_by_horizon"])):
                row = [pooled[f"{k}_by_horizon"][h] for k in ("count", "crossing_rate", "quantile_crps")]
                for k in QUANTILE_LEVEL_KEYS + QUANTILE_PAIR_KEYS:
                    row += list(pooled[f"{k}_by_horizon"][h])
                wr.writerow([g, h] + [repr(float(v)) for v in row])
    return {"npz": npz_path, "csv": csv_path}
