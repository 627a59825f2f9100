"""Split-conformal prediction intervals: calibrated error bars from one pass over a held-out split.

`ensemble_forecast` gives the interval between sorted MC-dropout members, whose nominal coverage holds only if members and
truth are exchangeable -- and `evaluate_ensemble` shows that they are not.  Split-conformal calibration needs no such
assumption about the model: record the forecast errors ("nonconformity scores") of a calibration split (the reference's
`val` split), cell by cell, and take as half-width the ceil((n + 1)(1 - alpha))-th smallest of a cell's n scores.  If the
calibration windows and the window to be forecast are exchangeable, the interval covers the truth with probability at least
1 - alpha, whatever the model; forecasting costs one forward.

  * `ConformalCalibrator.update` writes a batch's scores into a score store on the device (`tecm_conformal_scores`),
    `fit` selects the quantiles there (`tecm_column_select`, an exact radix select -- nothing is sorted and the store, 300 MB
    at the test split's size, never goes to the host) and returns a `ConformalIntervals`.
  * Groups (`window_groups_by_index`: storm level; `window_groups_by_slot`: time of day) give group-conditional
    ("Mondrian") intervals: every group has quantiles of its own, from its own windows.
  * With `members=K` the centre is the MC-dropout ensemble's mean and its standard deviation scales the score
    ("conformalised MC dropout"): the interval is mean +- q * max(std, sigma_min), wider where the members disagree.
  * `mode="absolute"` scores |y - p| and gives symmetric intervals; `mode="signed"` scores y - p and takes a lower and an
    upper quantile at alpha / 2 each, for errors that are skewed.

`IntervalMetrics` (src/evaluation/metrics.py, `tecm_interval_stats`) scores intervals on a split: coverage per (group,
horizon, node), on which side the misses fall, width and Winkler score.

Not covered: merging a score store across ranks.  Calibration is one pass on one device (the store of a split is one
tensor); `evaluate_conformal` merges its additive statistics across ranks like the other evaluations.
"""
from __future__ import annotations

import csv
import math
import os
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from .devcheck import check_device_errors, error_word
from .evaluate import _score_pass, check_grid
from .loop import _batches

MODES = ("absolute", "signed")
SIGMA_MIN = 1e-3            # TECU: the floor of the per-sample scale
TEC_MIN, TEC_MAX = 0.0, 200.0


def _alpha_fraction(alpha) -> Fraction:
    a = alpha if isinstance(alpha, Fraction) else Fraction(str(alpha))
    if not 0 < a < 1:
        raise ValueError(f"alpha must lie in (0, 1), got {alpha}")
    return a


def conformal_ranks(n: int, alpha, mode: str = "absolute") -> Tuple[int, ...]:
    """The 1-based ranks, among n calibration scores, of the quantiles of a split-conformal interval at miscoverage alpha:
    ("absolute") one rank ceil((n + 1)(1 - alpha)); ("signed") two, floor((n + 1) alpha / 2) and ceil((n + 1)(1 - alpha / 2)).
    Exact rational arithmetic on the decimal `alpha` as written (`Fraction(str(alpha))`), so that a product that is a whole
    number -- (19, 0.1): 20 * 9 / 10 = 18 -- is never rounded past it.  An upper rank of n + 1 (too few scores:
    n < ceil(1 / alpha) - 1) means +inf, a lower rank of 0 means -inf; `tecm_column_select` returns exactly those."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    n = int(n)
    if n < 0:
        raise ValueError(f"n must not be negative, got {n}")
    a = _alpha_fraction(alpha)
    if mode == "absolute":
        return (math.ceil((n + 1) * (1 - a)),)
    return (math.floor((n + 1) * a / 2), math.ceil((n + 1) * (1 - a / 2)))


class ConformalIntervals:
    """The calibrated quantiles: `q_lo`, `q_hi` (G, H, N) float32 numpy arrays in the score's units (TECU, or multiples of the
    per-sample scale) with q_lo = -q_hi in the absolute mode, `alpha`, `mode`, `counts` (G) calibration windows per group,
    `sigma_min`, `scaled` (whether the scores were divided by a per-sample scale) and the target scaler's `mean` / `scale`
    ((0, 1) and `clip` False without a scaler).  A sample's interval is [p + q_lo w, p + q_hi w] with p the forecast in
    physical units and w = max(sigma, sigma_min), or 1."""

    def __init__(self, q_lo, q_hi, alpha: float, mode: str, counts, sigma_min: float = SIGMA_MIN, scaled: bool = False,
                 mean: float = 0.0, scale: float = 1.0, clip: bool = False):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        self.q_lo = np.ascontiguousarray(q_lo, dtype=np.float32)
        self.q_hi = np.ascontiguousarray(q_hi, dtype=np.float32)
        if self.q_hi.ndim != 3 or self.q_lo.shape != self.q_hi.shape:
            raise ValueError(f"q_lo and q_hi must both be (G, H, N), got {self.q_lo.shape} and {self.q_hi.shape}")
        self.alpha, self.mode = float(alpha), mode
        self.counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        if self.counts.shape[0] != self.q_hi.shape[0]:
            raise ValueError("counts must hold one number per group")
        self.sigma_min, self.scaled = float(sigma_min), bool(scaled)
        self.mean, self.scale, self.clip = float(mean), float(scale), bool(clip)
        self._device: Dict[str, Tuple[Optional[torch.Tensor], torch.Tensor]] = {}

    @property
    def num_groups(self) -> int:
        return self.q_hi.shape[0]

    @property
    def scaler(self) -> Optional[Tuple[float, float]]:
        return (self.mean, self.scale) if self.clip else None

    @property
    def finite(self) -> bool:
        """Whether every group had enough calibration windows for a finite interval at this alpha."""
        return bool(np.isfinite(self.q_lo).all() and np.isfinite(self.q_hi).all())

    def on(self, device) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        """(q_lo, q_hi) as contiguous device tensors, q_lo None in the absolute mode: what `IntervalMetrics.update` takes."""
        key = str(torch.device(device))
        if key not in self._device:
            hi = torch.from_numpy(self.q_hi).to(device)
            lo = torch.from_numpy(self.q_lo).to(device) if self.mode == "signed" else None
            self._device[key] = (lo, hi)
        return self._device[key]

    def save(self, path: str) -> str:
        """One `.npz` of numpy arrays only (loads without pickle)."""
        np.savez(path, q_lo=self.q_lo, q_hi=self.q_hi, alpha=np.float64(self.alpha), mode=np.asarray(self.mode),
                 counts=self.counts, sigma_min=np.float64(self.sigma_min), scaled=np.asarray(self.scaled),
                 mean=np.float64(self.mean), scale=np.float64(self.scale), clip=np.asarray(self.clip))
        return path if path.endswith(".npz") else path + ".npz"

    @classmethod
    def load(cls, path: str) -> "ConformalIntervals":
        with np.load(path, allow_pickle=False) as z:
            return cls(z["q_lo"], z["q_hi"], float(z["alpha"]), str(z["mode"]), z["counts"], float(z["sigma_min"]),
                       bool(z["scaled"]), float(z["mean"]), float(z["scale"]), bool(z["clip"]))


class ConformalCalibrator:
    """The score store of one calibration pass: `capacity` rows of H*N float32 scores and one int32 group id per row, on the
    device.  update() appends a batch (`tecm_conformal_scores`), fit(alpha) selects the quantiles (`tecm_column_select`)."""

    def __init__(self, num_horizons: int, num_nodes: int, capacity: int, num_groups: int = 1, scaler=None,
                 mode: str = "absolute", device: Union[str, torch.device] = "cuda", sigma_min: float = SIGMA_MIN):
        from src.evaluation.metrics import _scaler_params
        self.H, self.I, self.G, self.capacity = int(num_horizons), int(num_nodes), int(num_groups), int(capacity)
        if min(self.H, self.I, self.G, self.capacity) < 1:
            raise ValueError("ConformalCalibrator needs at least one horizon, node, group and row")
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        self.mode, self.sigma_min = mode, float(sigma_min)
        self.scaler = _scaler_params(scaler)
        self.scores = torch.empty(self.capacity, self.H * self.I, device=device, dtype=torch.float32)
        self.groups = torch.zeros(self.capacity, device=device, dtype=torch.int32)
        self.rows = 0
        self.scaled: Optional[bool] = None

    def reset(self) -> None:
        self.rows, self.scaled = 0, None

    def update(self, y_pred_scaled: torch.Tensor, y_true_scaled: torch.Tensor, groups: Optional[torch.Tensor] = None,
               sigma: Optional[torch.Tensor] = None) -> None:
        """Append the scores of a batch: pred and truth (S, H, N) or (S, H, N, 1) in scaled units, read in place (the model's
        permuted output view needs no copy); groups (S) int32 on the device or None (group 0); sigma (S, H, N) in physical
        units or None -- every update of one calibration with it, or none."""
        from src.evaluation.metrics import _as_shi
        p, S, H, I, ps, ph, pi = _as_shi(y_pred_scaled, "y_pred")
        t, S2, H2, I2, ts, th, ti = _as_shi(y_true_scaled, "y_true")
        if (S, H, I) != (S2, H2, I2) or H != self.H or I != self.I:
            raise ValueError(f"shape mismatch: pred {tuple(y_pred_scaled.shape)}, true {tuple(y_true_scaled.shape)}, "
                             f"horizons {self.H}, nodes {self.I}")
        if self.rows + S > self.capacity:
            raise ValueError(f"the score store holds {self.capacity} rows: {self.rows} stored, {S} more do not fit")
        if self.scaled is not None and self.scaled != (sigma is not None):
            raise ValueError("either every update of a calibration has a sigma or none has")
        sg = None
        if sigma is not None:
            g_, S3, H3, I3, gs, gh, gi = _as_shi(sigma, "sigma")
            if (S3, H3, I3) != (S, H, I):
                raise ValueError(f"sigma must have the shape of pred, got {tuple(sigma.shape)}")
            sg = g_.as_strided((S, H, I), (gs, gh, gi))
        if groups is not None:
            if groups.dtype != torch.int32 or groups.shape != (S,):
                raise ValueError(f"groups must be int32 with one id per sample: {tuple(groups.shape)} for {S} samples")
            self.groups[self.rows:self.rows + S].copy_(groups)
        else:
            self.groups[self.rows:self.rows + S].zero_()
        mean, scale = self.scaler if self.scaler is not None else (0.0, 1.0)
        ops.conformal_scores(p.as_strided((S, H, I), (ps, ph, pi)), t.as_strided((S, H, I), (ts, th, ti)), self.scores,
                             self.rows, mode=self.mode, sigma=sg, sigma_min=self.sigma_min, mean=mean, scale=scale,
                             clip=(TEC_MIN, TEC_MAX) if self.scaler is not None else None)
        self.rows += S
        self.scaled = sigma is not None

    def fit(self, alpha=0.1):
        """The intervals at miscoverage `alpha` -- a `ConformalIntervals`; a list of them for a sequence of alphas (at most 8
        in the absolute and 4 in the signed mode), still from one selection.  One `bincount` of the stored group ids and one
        host synchronisation for the ranks, then ONE `tecm_column_select` call over the store.  An id outside [0, G) raises
        `TecmError`; a group with too few windows gets infinite quantiles (`ConformalIntervals.finite`)."""
        if self.rows == 0:
            raise ValueError("fit() before any update()")
        single = isinstance(alpha, (float, int, str, Fraction))
        alphas = [alpha] if single else list(alpha)
        per = 1 if self.mode == "absolute" else 2
        if not alphas or per * len(alphas) > ops._lib.TECM_SELECT_MAX_Q:
            raise ValueError(f"between 1 and {ops._lib.TECM_SELECT_MAX_Q // per} alphas per fit, got {len(alphas)}")
        ids = self.groups[:self.rows]
        inside = (ids >= 0) & (ids < self.G)
        counts = torch.bincount(ids[inside].to(torch.int64), minlength=self.G).cpu().numpy()       # the host sync
        ranks = np.array([[r for a in alphas for r in conformal_ranks(int(n), a, self.mode)] for n in counts], dtype=np.int32)
        errs = error_word(self.scores.device)
        out = ops.column_select(self.scores[:self.rows], torch.from_numpy(ranks).to(self.scores.device),
                                ids, errs.ptr())                                     # (Q, G, H*N)
        errs.post()
        check_device_errors(self.scores.device)
        q = out.cpu().numpy().reshape(len(alphas), per, self.G, self.H, self.I)
        mean, scale = self.scaler if self.scaler is not None else (0.0, 1.0)
        fitted = []
        for n, a in enumerate(alphas):
            q_hi = q[n, per - 1]
            q_lo = q[n, 0] if self.mode == "signed" else -q_hi
            fitted.append(ConformalIntervals(q_lo, q_hi, float(_alpha_fraction(a)), self.mode, counts, self.sigma_min,
                                             bool(self.scaled), mean, scale, self.scaler is not None))
        return fitted[0] if single else fitted


def _centre_and_sigma(model, x, tf, edge_index, edge_weight, out, y, members, seed, chunk, scaler):
    """The forecast the intervals are centred on, in scaled units, and its per-sample scale: the model's `eval()` output and
    None, or with `members=K` the MC-dropout ensemble's mean_raw and std (`EnsembleMetrics.update`, seeds of
    `ensemble_members`)."""
    if members is None:
        return out, None
    from src.evaluation.metrics import EnsembleMetrics
    from .ensemble import ensemble_members
    mem = ensemble_members(model, x, tf, edge_index, int(members), seed, chunk, edge_weight)
    K, B, H, N = mem.shape
    em = EnsembleMetrics(H, N, K, 1, scaler, 0, device=mem.device)
    truth = y if y is not None else torch.zeros(1, device=mem.device, dtype=torch.float32).expand(B, H, N)
    got = em.update(mem, truth, None, outputs=("mean_raw", "std"))
    return got["mean_raw"], got["std"]


@torch.no_grad()
def calibrate_conformal(model: torch.nn.Module, dataset, edge_index: torch.Tensor, batch_size: int, alpha=0.1, scaler=None,
                        groups: Optional[torch.Tensor] = None, num_groups: int = 1, mode: str = "absolute",
                        members: Optional[int] = None, seed: int = 0, order: Optional[Sequence[int]] = None,
                        edge_weight: Optional[torch.Tensor] = None):
    """One `eval()` no-grad pass over a calibration split (the reference's `val` split -- NOT the split the model was
    trained on, and not the one to be scored) and `ConformalCalibrator.fit(alpha)`: a `ConformalIntervals`, or a list for a
    sequence of alphas.  `groups` holds one int32 id in [0, num_groups) per DATASET index on the device, as in
    `evaluate_maps`; `order` restricts or reorders the windows.  With `members=K` (at least 2) every batch also runs K
    training-mode forwards: the centre is the ensemble's mean_raw, the scale its std.  One device, one pass: a score store
    is not merged across ranks."""
    if groups is not None and (groups.dtype != torch.int32 or groups.shape != (len(dataset),)):
        raise ValueError(f"groups must be an int32 tensor with one id per dataset index ({len(dataset)})")
    total = len(dataset) if order is None else len(list(order))
    if total == 0:
        raise ValueError("calibrate_conformal() on an empty dataset")
    was_training = model.training
    model.eval()
    cal = None
    try:
        for ordinal, chunk in enumerate(_batches(len(dataset), batch_size, order)):
            x, tf, y = dataset.batch(chunk)
            out = model(x, tf, edge_index, edge_weight)
            if cal is None:
                cal = ConformalCalibrator(out.shape[1], out.shape[2], total, int(num_groups), scaler, mode, out.device)
            ids = None
            if groups is not None:
                ids = groups[torch.as_tensor(chunk, dtype=torch.int64).to(groups.device, non_blocking=True)]
            centre, sigma = _centre_and_sigma(model, x, tf, edge_index, edge_weight, out, y, members, seed, ordinal, scaler)
            cal.update(centre, y, ids, sigma)
    finally:
        model.train(was_training)
    return cal.fit(alpha)


@torch.no_grad()
def conformal_forecast(model: torch.nn.Module, x: torch.Tensor, tf: torch.Tensor, edge_index: torch.Tensor,
                       intervals: ConformalIntervals, groups: Optional[torch.Tensor] = None, members: Optional[int] = None,
                       seed: int = 0, edge_weight: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """A forecast with its calibrated error bar: {"mean", "lo", "hi"}, device tensors (B, L_out, N) in TECU (scaled units
    if the intervals were calibrated without a scaler).  One `eval()` forward -- plus K training-mode ones with `members=K`,
    which intervals calibrated with members need.  `groups` (B) int32 on the device picks every sample's group for
    group-conditional intervals (None: group 0)."""
    from src.evaluation.metrics import IntervalMetrics
    if intervals.scaled != (members is not None):
        raise ValueError("intervals calibrated with members need members= here, and the other way round")
    was_training = model.training
    model.eval()
    try:
        out = model(x, tf, edge_index, edge_weight)
        centre, sigma = _centre_and_sigma(model, x, tf, edge_index, edge_weight, out, None, members, seed, 0, intervals.scaler)
    finally:
        model.train(was_training)
    im = IntervalMetrics(out.shape[1], out.shape[2], intervals.num_groups, intervals.scaler, intervals.alpha, intervals.mode,
                         out.device, intervals.sigma_min)
    got = im.update(centre, None, intervals.on(out.device), groups, sigma, outputs=("mid", "lo", "hi"))
    if groups is not None:
        check_device_errors(out.device)
    return {"mean": got["mid"], "lo": got["lo"], "hi": got["hi"]}


@torch.no_grad()
def evaluate_conformal(model: torch.nn.Module, dataset, edge_index: torch.Tensor, batch_size: int,
                       intervals: ConformalIntervals, groups: Optional[torch.Tensor] = None, num_groups: int = 1,
                       baselines: Sequence[str] = ("mean",), members: Optional[int] = None, seed: int = 0,
                       edge_weight: Optional[torch.Tensor] = None, order: Optional[Sequence[int]] = None, group=None,
                       first_chunk: int = 0):
    """`evaluate_maps` plus the intervals: returns (results, maps, conf).  The same single pass (`_score_pass`), so `results`
    and `maps` are `evaluate_maps`' entries bit for bit (scored with the scaler the intervals were calibrated with); per
    batch the intervals are scored too (`IntervalMetrics`, whose `compute()` is `conf`).  `groups` / `num_groups` stratify
    the statistics as in `evaluate_maps`; group-conditional intervals need the grouping they were calibrated with, intervals
    of one group serve any.  `members`, `seed` as in `calibrate_conformal`, with `first_chunk` as in `evaluate_ensemble`;
    `order` and `group` as in `evaluate_maps`: the statistics are sums and merge across ranks."""
    from src.evaluation.metrics import IntervalMetrics
    if groups is not None and (groups.dtype != torch.int32 or groups.shape != (len(dataset),)):
        raise ValueError(f"groups must be an int32 tensor with one id per dataset index ({len(dataset)})")
    if intervals.num_groups not in (1, int(num_groups)):
        raise ValueError(f"intervals of {intervals.num_groups} groups do not fit num_groups = {num_groups}")
    if intervals.scaled != (members is not None):
        raise ValueError("intervals calibrated with members need members= here, and the other way round")
    scaler = intervals.scaler
    box: List[IntervalMetrics] = []

    def per_batch(ordinal, x, tf, y, out, ids):
        if not box:
            box.append(IntervalMetrics(out.shape[1], out.shape[2], int(num_groups), scaler, intervals.alpha, intervals.mode,
                                       out.device, intervals.sigma_min))
        centre, sigma = _centre_and_sigma(model, x, tf, edge_index, edge_weight, out, y, members, seed,
                                          int(first_chunk) + ordinal, scaler)
        box[0].update(centre, y, intervals.on(out.device), ids, sigma)

    hms, mms = _score_pass(model, dataset, edge_index, batch_size, scaler, baselines, edge_weight, order, groups,
                           int(num_groups), per_batch)
    if not hms:
        raise ValueError("evaluate_conformal() on an empty dataset")
    results = {name: hm.merge_(group).compute() for name, hm in hms.items()}
    maps = {name: mm.merge_(group).compute() for name, mm in mms.items()}
    conf = box[0].merge_(group).compute()
    check_device_errors(box[0].stats.device)
    return results, maps, conf


CSV_COLUMNS = ("count", "coverage", "nominal_coverage", "miss_below", "miss_above", "interval_width", "interval_score")


def write_conformal(conf: Dict[str, object], output_dir: str, grid: Optional[Sequence[int]] = None) -> Dict[str, str]:
    """The files of `evaluate_conformal`'s third result: `conformal_maps.npz` with one (G, H, N) array per key of
    `INTERVAL_KEYS` -- (G, H, *grid) when `grid`, e.g. (41, 71), is given -- plus `nominal_coverage`; and
    `conformal_by_horizon.csv` with one row per group and horizon: that group's statistics pooled over the nodes
    (CSV_COLUMNS).  numpy and the standard library only.  Returns the two paths."""
    from src.evaluation.metrics import INTERVAL_KEYS
    os.makedirs(output_dir, exist_ok=True)
    arrays = {}
    for k in INTERVAL_KEYS:
        a = np.asarray(conf[k])
        if grid is not None:
            check_grid(grid, a.shape[2])
            a = a.reshape(a.shape[0], a.shape[1], *[int(d) for d in grid])
        arrays[k] = a
    arrays["nominal_coverage"] = np.asarray(float(conf["nominal_coverage"]))
    npz_path = os.path.join(output_dir, "conformal_maps.npz")
    np.savez_compressed(npz_path, **arrays)
    csv_path = os.path.join(output_dir, "conformal_by_horizon.csv")
    with open(csv_path, "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow(["group", "horizon"] + list(CSV_COLUMNS))
        for g, pooled in enumerate(conf["by_group"]):
            for h in range(len(pooled["coverage_by_horizon"])):
                wr.writerow([g, h] + [repr(float(conf["nominal_coverage"] if k == "nominal_coverage"
                                                 else pooled[f"{k}_by_horizon"][h])) for k in CSV_COLUMNS])
    return {"npz": npz_path, "csv": csv_path}
