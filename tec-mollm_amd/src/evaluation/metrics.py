"""Device-side mirror of the reference's `src/evaluation/metrics.py` (`/root/reference/src/evaluation/metrics.py`).

`evaluate_horizons` (:119-183) is what `validate()` calls once per epoch after collecting every batch's
predictions on the host (`train.py:153-166`, one `.cpu().numpy()` sync per batch).  Here the per-horizon
sufficient statistics are accumulated on the GPU batch by batch (`HorizonMetrics.update`, one kernel,
no sync, reads the model's permuted output view in place) and the 4 metrics x L_out horizons are derived
from 8*L_out doubles in `compute()` -- the only device->host copy of the whole evaluation.

`MapMetrics` keeps the same statistics per (group, horizon, node) cell instead of per horizon (`tecm_metrics_map`), and
`derive` turns statistics of any leading shape into the metrics, NaN where a cell saw no sample.  `EnsembleMetrics` scores a
K-member ensemble per cell the same way (`tecm_ensemble_stats`: CRPS, spread, coverage, rank histogram; `derive_ensemble`).
`IntervalMetrics` scores conformal prediction intervals per cell (`tecm_interval_stats`: coverage, side of the misses, width,
Winkler score; `derive_intervals`); the intervals themselves come from `tecmollm/conformal.py`.  `EventMetrics` counts events
per cell and threshold (`tecm_event_hist`, `tecm_event_fss`: contingency tables, the member histogram behind Brier / reliability
/ ROC, the sums of the fractions skill score; `derive_events`, `derive_fss`); thresholds and the pass are in `tecmollm/events.py`.
`FieldMetrics` scores an ensemble's members as maps per (group, horizon) (`tecm_field_scores`: energy score, variogram score
by class of node pairs; `derive_fields`); the class matrix and the files are in `tecmollm/fields.py`.

Same numbers as the reference: inverse StandardScaler transform, non-finite guards, clip of predictions
to [0, 200] TECU, MAE / RMSE / R^2 (sklearn semantics) / Pearson r per horizon and their averages.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch

from tecmollm import _lib
from tecmollm._lib import TecmError, TecmMetrics, TecmMetricsMap, check, lib, stream_ptr

TEC_MIN, TEC_MAX = 0.0, 200.0           # metrics.py:50


def _scaler_params(scaler) -> Optional[Tuple[float, float]]:
    """Accepts None, a (mean, scale) pair, a fitted sklearn StandardScaler, or a joblib path to one (:148-150)."""
    if scaler is None:
        return None
    if isinstance(scaler, str):
        import joblib
        scaler = joblib.load(scaler)
    if isinstance(scaler, (tuple, list)):
        return float(scaler[0]), float(scaler[1])
    mean = np.asarray(scaler.mean_).reshape(-1)
    scale = np.asarray(scaler.scale_).reshape(-1)
    if mean.size != 1 or scale.size != 1:
        raise ValueError("the target scaler must be fitted on a single feature (metrics.py:26-37)")
    return float(mean[0]), float(scale[0])


def _as_shi(t: torch.Tensor, name: str):
    """(S, H, ...) tensor -> element strides (s, h, i) with the trailing dims flattened to one index."""
    _lib.require_gpu_tensor(t, name)
    if t.dim() < 2:
        raise ValueError(f"{name} must be (samples, horizons, ...)")
    S, H = t.shape[0], t.shape[1]
    rest = t.shape[2:]
    I = int(np.prod(rest)) if rest else 1
    # the trailing dims must collapse to a single stride (true for contiguous tensors and for the
    # (B, L_out, N, 1) permuted view the model returns)
    stride_i, expect = None, None
    for size, st in zip(reversed(rest), reversed(t.stride()[2:])):
        if size == 1:
            continue
        if stride_i is None:
            stride_i, expect = st, st * size
        elif st != expect:
            return _as_shi(t.contiguous(), name)
        else:
            expect = st * size
    return t, S, H, I, t.stride(0), t.stride(1), (stride_i if stride_i is not None else 1)


class HorizonMetrics:
    """Streaming `evaluate_horizons`: update(pred, true) per batch on the device, compute() at the end."""

    def __init__(self, num_horizons: int, scaler=None, device: Union[str, torch.device] = "cuda"):
        self.H = int(num_horizons)
        self.scaler = _scaler_params(scaler)
        self.stats = torch.zeros(self.H, _lib.TECM_METRIC_STATS, device=device, dtype=torch.float64)

    def reset(self) -> None:
        self.stats.zero_()

    def update(self, y_pred_scaled: torch.Tensor, y_true_scaled: torch.Tensor) -> None:
        p, S, H, I, ps, ph, pi = _as_shi(y_pred_scaled, "y_pred")
        t, S2, H2, I2, ts, th, ti = _as_shi(y_true_scaled, "y_true")
        if (S, H, I) != (S2, H2, I2) or H != self.H:
            raise ValueError(f"shape mismatch: pred {tuple(y_pred_scaled.shape)}, true {tuple(y_true_scaled.shape)}, "
                             f"horizons {self.H}")
        mean, scale = self.scaler if self.scaler is not None else (0.0, 1.0)
        m = TecmMetrics(pred=p.data_ptr(), p_stride_s=ps, p_stride_h=ph, p_stride_i=pi,
                        target=t.data_ptr(), t_stride_s=ts, t_stride_h=th, t_stride_i=ti,
                        S=S, H=H, I=I, mean=mean, scale=scale, clip_lo=TEC_MIN, clip_hi=TEC_MAX,
                        clip=1 if self.scaler is not None else 0, stats=self.stats.data_ptr())
        check(lib().tecm_metrics_accumulate(C.byref(m), stream_ptr()), "tecm_metrics_accumulate")

    def merge_(self, group=None) -> "HorizonMetrics":
        """Sum the (H, 8) statistics over the ranks of `group` (None: the default process group) with one all-reduce,
        in place.  Every statistic is a plain sum over (sample, node) pairs, so ranks that each fed their own shard of a
        split end up with the statistics -- and hence the metrics -- of the whole split; the reference lets rank 0
        report its own shard only (train.py:153-166, :389-410).  Without an initialised process group this is a no-op."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.stats, op=dist.ReduceOp.SUM, group=group)
        return self

    def compute(self) -> Dict[str, object]:
        st = self.stats.cpu().numpy()
        per = []
        for n, st_, sp, stt, spp, stp, sabs, ssq in st:
            if n == 0:
                raise ValueError("HorizonMetrics.compute() before any update()")
            mae, rmse = sabs / n, math.sqrt(ssq / n)
            ss_tot = stt - st_ * st_ / n
            ss_p = spp - sp * sp / n
            # a constant series must read as exactly zero variance (np.std(...) > 0 test, metrics.py:73):
            # the one-pass form leaves rounding noise of order eps * sum(t^2)
            var_floor = 64 * np.finfo(np.float64).eps
            if ss_tot <= var_floor * max(stt, 1e-300):
                ss_tot = 0.0
            if ss_p <= var_floor * max(spp, 1e-300):
                ss_p = 0.0
            if ss_tot != 0.0:
                r2 = 1.0 - ssq / ss_tot
            else:
                r2 = 1.0 if ssq == 0.0 else 0.0
            if ss_tot > 0 and ss_p > 0:
                pear = (stp - st_ * sp / n) / math.sqrt(ss_tot * ss_p)
                pear = max(-1.0, min(1.0, pear))
            else:
                pear = 0.0
            per.append({"mae": mae, "rmse": rmse, "r2_score": r2, "pearson_r": pear})
        return {
            "mae_avg": float(np.mean([m["mae"] for m in per])),
            "rmse_avg": float(np.mean([m["rmse"] for m in per])),
            "r2_score_avg": float(np.mean([m["r2_score"] for m in per])),
            "pearson_r_avg": float(np.mean([m["pearson_r"] for m in per])),
            "mae_by_horizon": [m["mae"] for m in per],
            "rmse_by_horizon": [m["rmse"] for m in per],
            "r2_by_horizon": [m["r2_score"] for m in per],
            "pearson_by_horizon": [m["pearson_r"] for m in per],
        }


def derive(stats: np.ndarray) -> Dict[str, np.ndarray]:
    """(..., 8) float64 sufficient statistics -> {"count", "mae", "rmse", "bias", "r2_score", "pearson_r"}, arrays over the
    leading axes: `evaluate_metrics` (metrics.py:10-89) of every cell at once, with the variance floor and the
    degenerate-case rules of `HorizonMetrics.compute()` in the same operations and order.  `bias` is the mean of p - t.  A
    cell without samples (n = 0) reads NaN in every metric."""
    st = np.asarray(stats, dtype=np.float64)
    n, st_, sp, stt, spp, stp, sabs, ssq = np.moveaxis(st, -1, 0)
    var_floor = 64 * np.finfo(np.float64).eps
    with np.errstate(divide="ignore", invalid="ignore"):
        mae, rmse, bias = sabs / n, np.sqrt(ssq / n), (sp - st_) / n
        ss_tot = stt - st_ * st_ / n
        ss_p = spp - sp * sp / n
        ss_tot = np.where(ss_tot <= var_floor * np.maximum(stt, 1e-300), 0.0, ss_tot)
        ss_p = np.where(ss_p <= var_floor * np.maximum(spp, 1e-300), 0.0, ss_p)
        r2 = np.where(ss_tot != 0.0, 1.0 - ssq / ss_tot, np.where(ssq == 0.0, 1.0, 0.0))
        both = (ss_tot > 0) & (ss_p > 0)
        pear = np.where(both, np.clip((stp - st_ * sp / n) / np.sqrt(ss_tot * ss_p), -1.0, 1.0), 0.0)
    empty = n == 0
    out = {"count": n.copy(), "mae": mae, "rmse": rmse, "bias": bias, "r2_score": r2, "pearson_r": pear}
    for k in ("mae", "rmse", "bias", "r2_score", "pearson_r"):
        out[k] = np.where(empty, np.nan, out[k])
    return out


def _pooled(per: Dict[str, np.ndarray]) -> Dict[str, object]:
    """`derive` of (H, 8) rows -> the dict `HorizonMetrics.compute()` returns."""
    return {
        "mae_avg": float(np.mean(per["mae"])), "rmse_avg": float(np.mean(per["rmse"])),
        "r2_score_avg": float(np.mean(per["r2_score"])), "pearson_r_avg": float(np.mean(per["pearson_r"])),
        "mae_by_horizon": per["mae"].tolist(), "rmse_by_horizon": per["rmse"].tolist(),
        "r2_by_horizon": per["r2_score"].tolist(), "pearson_by_horizon": per["pearson_r"].tolist(),
    }


MAP_KEYS = ("count", "mae", "rmse", "bias", "r2_score", "pearson_r")


class MapMetrics:
    """`HorizonMetrics` one level down: the same eight statistics per cell (group of the sample, horizon, node), for error
    maps and for scores stratified by storm level or time of day.  update(pred, true, groups) per batch on the device (one
    kernel, `tecm_metrics_map`: no atomics, so the same batches give the same bits), compute() at the end."""

    def __init__(self, num_horizons: int, num_nodes: int, num_groups: int = 1, scaler=None,
                 device: Union[str, torch.device] = "cuda"):
        self.H, self.I, self.G = int(num_horizons), int(num_nodes), int(num_groups)
        if min(self.H, self.I, self.G) < 1:
            raise ValueError("MapMetrics needs at least one horizon, one node and one group")
        self.scaler = _scaler_params(scaler)
        # [g][h][k][i]: node-contiguous, the layout the kernel's lanes read and write
        self.stats = torch.zeros(self.G, self.H, _lib.TECM_METRIC_STATS, self.I, device=device, dtype=torch.float64)

    def reset(self) -> None:
        self.stats.zero_()

    def update(self, y_pred_scaled: torch.Tensor, y_true_scaled: torch.Tensor, groups: Optional[torch.Tensor] = None) -> None:
        from tecmollm import devcheck
        p, S, H, I, ps, ph, pi = _as_shi(y_pred_scaled, "y_pred")
        t, S2, H2, I2, ts, th, ti = _as_shi(y_true_scaled, "y_true")
        if (S, H, I) != (S2, H2, I2) or H != self.H or I != self.I:
            raise ValueError(f"shape mismatch: pred {tuple(y_pred_scaled.shape)}, true {tuple(y_true_scaled.shape)}, "
                             f"horizons {self.H}, nodes {self.I}")
        if groups is not None:
            _lib.require_gpu_tensor(groups, "groups", torch.int32)
            if groups.shape != (S,):
                raise ValueError(f"groups must hold one id per sample: {tuple(groups.shape)} for {S} samples")
            groups = groups.contiguous()
        mean, scale = self.scaler if self.scaler is not None else (0.0, 1.0)
        errs = devcheck.error_word(self.stats.device)
        m = TecmMetricsMap(pred=p.data_ptr(), p_stride_s=ps, p_stride_h=ph, p_stride_i=pi,
                           target=t.data_ptr(), t_stride_s=ts, t_stride_h=th, t_stride_i=ti,
                           S=S, H=H, G=self.G, I=I, mean=mean, scale=scale, clip_lo=TEC_MIN, clip_hi=TEC_MAX,
                           clip=1 if self.scaler is not None else 0, stats=self.stats.data_ptr(),
                           group=_lib.ptr(groups), err_flag=errs.ptr())
        check(lib().tecm_metrics_map(C.byref(m), stream_ptr()), "tecm_metrics_map")
        if groups is not None:
            errs.post()                        # only a group id can set the word here

    def merge_(self, group=None) -> "MapMetrics":
        """Sum the statistics over the ranks of `group` with one all-reduce, in place (see `HorizonMetrics.merge_`)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.stats, op=dist.ReduceOp.SUM, group=group)
        return self

    def collapse(self) -> np.ndarray:
        """The (H, 8) statistics summed over groups and nodes: what a `HorizonMetrics` fed the same batches holds."""
        return self.stats.sum(dim=(0, 3)).cpu().numpy()

    def compute(self) -> Dict[str, object]:
        """{"count", "mae", "rmse", "bias", "r2_score", "pearson_r"}: numpy (G, H, I) arrays, NaN where a cell saw no sample;
        "by_group": per group the `HorizonMetrics.compute()` dict of its statistics summed over the nodes (NaN for a group
        the split never visits)."""
        st = self.stats.permute(0, 1, 3, 2).cpu().numpy()                   # (G, H, I, 8)
        out: Dict[str, object] = dict(derive(st))
        out["by_group"] = [_pooled(derive(st[g].sum(axis=1))) for g in range(self.G)]
        return out


def evaluate_horizons(y_true_horizons_scaled, y_pred_horizons_scaled, target_scaler_path: Optional[str] = None,
                      device: Union[str, torch.device] = "cuda") -> Dict[str, object]:
    """Same signature and result dict as the reference (:119-183); arrays (S, L_out, ...) may be CUDA tensors
    (used in place) or numpy arrays / CPU tensors (uploaded first -- the arithmetic always runs on the GPU)."""
    def dev(a):
        t = torch.as_tensor(a)
        return t.to(device=device, dtype=torch.float32)
    t, p = dev(y_true_horizons_scaled), dev(y_pred_horizons_scaled)
    hm = HorizonMetrics(t.shape[1], target_scaler_path, device=t.device)
    hm.update(p, t)
    return hm.compute()


# ------------------------------------------------------------------------------------ ensembles
ENSEMBLE_KEYS = ("count", "crps", "fair_crps", "rmse_mean", "mae_mean", "bias_mean", "spread", "spread_skill", "coverage",
                 "interval_width")


def nominal_coverage(members: int, trim: int) -> float:
    """The share of the K + 1 equally likely ranks of the truth among K exchangeable members that lie inside the interval
    [x_(1+m), x_(K-m)]: (K - 2m - 1) / (K + 1)."""
    return (members - 2 * trim - 1) / (members + 1)


def derive_ensemble(stats: np.ndarray, hist: np.ndarray, members: int, trim: int = 0) -> Dict[str, np.ndarray]:
    """(..., 9) float64 sums [count, sum y, sum mu, sum (mu-y)^2, sum |mu-y|, sum var, sum A, sum D, sum width] and
    (..., K+1) rank counts -> the ENSEMBLE_KEYS, arrays over the leading axes, NaN where a cell saw no sample:
      crps = mean(A) - mean(D) / K^2                      fair_crps = mean(A) - mean(D) / (K (K - 1))
      rmse_mean, mae_mean, bias_mean: of the ensemble mean against the truth (bias = mean(mu - y))
      spread = sqrt(mean var)                             spread_skill = sqrt((K + 1) / K * mean var / MSE of the mean)
      coverage = share of ranks in [m + 1, K - m - 1]     interval_width = mean(x_(K-m) - x_(1+m))
    (1 for a spread_skill means the spread explains the error of the mean; it is inf or NaN where that error is 0)."""
    K, m = int(members), int(trim)
    st = np.asarray(stats, dtype=np.float64)
    hs = np.asarray(hist, dtype=np.float64)
    if st.shape[-1] != _lib.TECM_ENS_STATS or hs.shape[-1] != K + 1 or st.shape[:-1] != hs.shape[:-1]:
        raise ValueError(f"stats (..., 9) and hist (..., {K + 1}) do not fit: {st.shape}, {hs.shape}")
    if not (K >= 2 and 0 <= 2 * m < K - 1):
        raise ValueError(f"needs members >= 2 and 0 <= 2 * trim < members - 1 (members {K}, trim {m})")
    n, sy, smu, sse, sae, svar, sA, sD, sw = np.moveaxis(st, -1, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mse, mvar = sse / n, svar / n
        out = {"count": n.copy(),
               "crps": (sA - sD / (K * K)) / n, "fair_crps": (sA - sD / (K * (K - 1))) / n,
               "rmse_mean": np.sqrt(mse), "mae_mean": sae / n, "bias_mean": (smu - sy) / n,
               "spread": np.sqrt(mvar), "spread_skill": np.sqrt((K + 1) / K * mvar / mse),
               "coverage": hs[..., m + 1:K - m].sum(axis=-1) / n, "interval_width": sw / n}
    empty = n == 0
    for k in ENSEMBLE_KEYS[1:]:
        out[k] = np.where(empty, np.nan, out[k])
    return out


def _pooled_ensemble(per: Dict[str, np.ndarray]) -> Dict[str, object]:
    """`derive_ensemble` of (H, ...) rows -> per key its list by horizon and the average over the horizons."""
    out: Dict[str, object] = {"count_by_horizon": per["count"].tolist()}
    for k in ENSEMBLE_KEYS[1:]:
        out[f"{k}_by_horizon"] = per[k].tolist()
        out[f"{k}_avg"] = float(np.mean(per[k]))
    return out


class EnsembleMetrics:
    """Probabilistic scores of a K-member ensemble per cell (group of the sample, horizon, node): CRPS and fair CRPS, the
    error of the ensemble mean, spread, spread/skill, the coverage and width of the interval [x_(1+trim), x_(K-trim)] and
    the rank histogram.  update(members, true, groups) per batch on the device (one kernel, `tecm_ensemble_stats`: the
    members are not copied to the host, no atomics, so the same batches give the same bits), compute() at the end."""

    def __init__(self, num_horizons: int, num_nodes: int, members: int, num_groups: int = 1, scaler=None, trim: int = 0,
                 device: Union[str, torch.device] = "cuda"):
        self.H, self.I, self.K, self.G, self.trim = int(num_horizons), int(num_nodes), int(members), int(num_groups), int(trim)
        if min(self.H, self.I, self.G) < 1:
            raise ValueError("EnsembleMetrics needs at least one horizon, one node and one group")
        if not 2 <= self.K <= _lib.TECM_ENS_MAX_K:
            raise ValueError(f"members must lie in [2, {_lib.TECM_ENS_MAX_K}], got {self.K}")
        if not 0 <= 2 * self.trim < self.K - 1:
            raise ValueError(f"trim must satisfy 0 <= 2 * trim < members - 1 (members {self.K}, trim {self.trim})")
        self.scaler = _scaler_params(scaler)
        # [g][h][k][i] and [g][h][r][i]: node-contiguous, the layout the kernel's lanes read and write
        self.stats = torch.zeros(self.G, self.H, _lib.TECM_ENS_STATS, self.I, device=device, dtype=torch.float64)
        self.hist = torch.zeros(self.G, self.H, self.K + 1, self.I, device=device, dtype=torch.int32)

    @property
    def nominal_coverage(self) -> float:
        return nominal_coverage(self.K, self.trim)

    def reset(self) -> None:
        self.stats.zero_()
        self.hist.zero_()

    def update(self, members_scaled: torch.Tensor, y_true_scaled: torch.Tensor, groups: Optional[torch.Tensor] = None,
               outputs=()) -> Dict[str, torch.Tensor]:
        """members (K, S, H, N) or (K, S, H, N, 1) and the truth (S, H, N) or (S, H, N, 1), both in scaled units and read in
        place whatever their strides (node-contiguous members are the coalesced layout); groups (S) int32 or None.
        Returns the per-sample tensors named in `outputs` (`ops.ENSEMBLE_OUTPUTS`), each (S, H, N) float32: mean, std, lo,
        hi in physical units, mean_raw in scaled units."""
        from tecmollm import devcheck, ops
        m = members_scaled
        _lib.require_gpu_tensor(m, "members")
        if m.dim() == 5 and m.shape[-1] == 1:
            m = m.squeeze(-1)
        if m.dim() != 4:
            raise ValueError(f"members must be (K, S, H, N), got {tuple(members_scaled.shape)}")
        t, S, H, I, ts, th, ti = _as_shi(y_true_scaled, "y_true")
        if tuple(m.shape) != (self.K, S, H, I) or H != self.H or I != self.I:
            raise ValueError(f"shape mismatch: members {tuple(members_scaled.shape)}, true {tuple(y_true_scaled.shape)}, "
                             f"expected members {self.K}, horizons {self.H}, nodes {self.I}")
        if groups is not None:
            _lib.require_gpu_tensor(groups, "groups", torch.int32)
            if groups.shape != (S,):
                raise ValueError(f"groups must hold one id per sample: {tuple(groups.shape)} for {S} samples")
            groups = groups.contiguous()
        mean, scale = self.scaler if self.scaler is not None else (0.0, 1.0)
        errs = devcheck.error_word(self.stats.device)
        outs = {name: torch.empty(S, H, I, device=m.device, dtype=torch.float32) for name in outputs}
        ops.ensemble_stats(m, t.as_strided((S, H, I), (ts, th, ti)), self.stats, self.hist, trim=self.trim, mean=mean,
                           scale=scale, clip=(TEC_MIN, TEC_MAX) if self.scaler is not None else None, groups=groups,
                           err_flag=errs.ptr(), outputs=outs)
        if groups is not None:
            errs.post()                        # only a group id can set the word here
        return outs

    def merge_(self, group=None) -> "EnsembleMetrics":
        """Sum the statistics and the rank counts over the ranks of `group`, in place: both live in one buffer for the
        length of ONE all-reduce (the counts as float64, exact below 2^53).  See `HorizonMetrics.merge_`."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            n = self.stats.numel()
            flat = torch.cat([self.stats.reshape(-1), self.hist.reshape(-1).to(torch.float64)])
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
            self.stats.copy_(flat[:n].view_as(self.stats))
            self.hist.copy_(flat[n:].view_as(self.hist).to(torch.int32))
        return self

    def compute(self) -> Dict[str, object]:
        """The ENSEMBLE_KEYS as numpy (G, H, N) arrays, NaN where a cell saw no sample; "nominal_coverage" (a float);
        "rank_histogram" (G, H, K+1), the rank counts pooled over the nodes; "by_group": per group the scores of its
        statistics pooled over the nodes, by horizon and averaged over the horizons (NaN for a group never visited)."""
        st = self.stats.permute(0, 1, 3, 2).cpu().numpy()                   # (G, H, I, 9)
        hs = self.hist.permute(0, 1, 3, 2).cpu().numpy().astype(np.int64)   # (G, H, I, K+1)
        out: Dict[str, object] = dict(derive_ensemble(st, hs, self.K, self.trim))
        out["nominal_coverage"] = self.nominal_coverage
        out["rank_histogram"] = hs.sum(axis=2)
        out["by_group"] = [_pooled_ensemble(derive_ensemble(st[g].sum(axis=1), hs[g].sum(axis=1), self.K, self.trim))
                           for g in range(self.G)]
        return out


# ------------------------------------------------------------------------------------ conformal intervals
INTERVAL_KEYS = ("count", "coverage", "miss_below", "miss_above", "interval_width", "interval_score")


def derive_intervals(stats: np.ndarray) -> Dict[str, np.ndarray]:
    """(..., 6) float64 sums [count, covered, below, above, sum width, sum Winkler] -> the INTERVAL_KEYS, arrays over the
    leading axes, NaN where a cell saw no sample: coverage, miss_below and miss_above are the shares of the samples inside,
    under and over their interval (they add up to 1), interval_width and interval_score (Winkler) the means."""
    st = np.asarray(stats, dtype=np.float64)
    if st.shape[-1] != _lib.TECM_INTERVAL_STATS:
        raise ValueError(f"stats must be (..., {_lib.TECM_INTERVAL_STATS}), got {st.shape}")
    n, cov, below, above, sw, ss = np.moveaxis(st, -1, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"count": n.copy(), "coverage": cov / n, "miss_below": below / n, "miss_above": above / n,
               "interval_width": sw / n, "interval_score": ss / n}
    empty = n == 0
    for k in INTERVAL_KEYS[1:]:
        out[k] = np.where(empty, np.nan, out[k])
    return out


def _pooled_intervals(per: Dict[str, np.ndarray]) -> Dict[str, object]:
    """`derive_intervals` of (H, ...) rows -> per key its list by horizon and the average over the horizons."""
    out: Dict[str, object] = {"count_by_horizon": per["count"].tolist()}
    for k in INTERVAL_KEYS[1:]:
        out[f"{k}_by_horizon"] = per[k].tolist()
        out[f"{k}_avg"] = float(np.mean(per[k]))
    return out


class IntervalMetrics:
    """Coverage, the side of the misses, width and Winkler score of conformal intervals per cell (group of the sample,
    horizon, node).  update(pred, true, q, groups) per batch on the device (one kernel, `tecm_interval_stats`: the score of
    every sample is the one `ConformalCalibrator` stores, no atomics, so the same batches give the same bits), compute() at
    the end.  It mirrors `EnsembleMetrics`."""

    def __init__(self, num_horizons: int, num_nodes: int, num_groups: int = 1, scaler=None, alpha: float = 0.1,
                 mode: str = "absolute", device: Union[str, torch.device] = "cuda", sigma_min: float = 1e-3):
        from tecmollm import ops
        self.H, self.I, self.G = int(num_horizons), int(num_nodes), int(num_groups)
        if min(self.H, self.I, self.G) < 1:
            raise ValueError("IntervalMetrics needs at least one horizon, one node and one group")
        self.alpha = float(alpha)
        if not 0.0 < self.alpha < 1.0:
            raise ValueError(f"alpha must lie in (0, 1), got {alpha}")
        if mode not in ops.CONFORMAL_MODES:
            raise ValueError(f"mode must be one of {sorted(ops.CONFORMAL_MODES)}, got {mode!r}")
        self.mode, self.sigma_min = mode, float(sigma_min)
        self.scaler = _scaler_params(scaler)
        # [g][h][k][i]: node-contiguous, the layout the kernel's lanes read and write
        self.stats = torch.zeros(self.G, self.H, _lib.TECM_INTERVAL_STATS, self.I, device=device, dtype=torch.float64)

    @property
    def nominal_coverage(self) -> float:
        return 1.0 - self.alpha

    def reset(self) -> None:
        self.stats.zero_()

    def update(self, y_pred_scaled: torch.Tensor, y_true_scaled: Optional[torch.Tensor], q,
               groups: Optional[torch.Tensor] = None, sigma: Optional[torch.Tensor] = None,
               outputs=()) -> Dict[str, torch.Tensor]:
        """pred and truth (S, H, N) or (S, H, N, 1) in scaled units, read in place whatever their strides; `q` = (q_lo, q_hi),
        contiguous float32 device tensors (1 or G, H, N) with q_lo None in the absolute mode (`ConformalIntervals.on(device)`);
        groups (S) int32 or None; sigma (S, H, N) in physical units or None.  With the truth None nothing is accumulated and
        only the per-sample tensors are made.  Returns the tensors named in `outputs` (`ops.INTERVAL_OUTPUTS`), each (S, H, N)
        float32 in physical units: lo, hi and mid, the centre of the interval."""
        from tecmollm import devcheck, ops
        p, S, H, I, ps, ph, pi = _as_shi(y_pred_scaled, "y_pred")
        if H != self.H or I != self.I:
            raise ValueError(f"shape mismatch: pred {tuple(y_pred_scaled.shape)}, horizons {self.H}, nodes {self.I}")
        views = [p.as_strided((S, H, I), (ps, ph, pi))]
        for t, name in ((y_true_scaled, "y_true"), (sigma, "sigma")):
            if t is None:
                views.append(None)
                continue
            t, S2, H2, I2, ts, th, ti = _as_shi(t, name)
            if (S2, H2, I2) != (S, H, I):
                raise ValueError(f"shape mismatch: pred {tuple(y_pred_scaled.shape)}, {name} {tuple(t.shape)}")
            views.append(t.as_strided((S, H, I), (ts, th, ti)))
        if groups is not None:
            _lib.require_gpu_tensor(groups, "groups", torch.int32)
            if groups.shape != (S,):
                raise ValueError(f"groups must hold one id per sample: {tuple(groups.shape)} for {S} samples")
            groups = groups.contiguous()
        q_lo, q_hi = q
        mean, scale = self.scaler if self.scaler is not None else (0.0, 1.0)
        errs = devcheck.error_word(self.stats.device)
        outs = {name: torch.empty(S, H, I, device=p.device, dtype=torch.float32) for name in outputs}
        ops.interval_stats(views[0], views[1], q_lo, q_hi, self.stats, alpha=self.alpha, mode=self.mode, sigma=views[2],
                           sigma_min=self.sigma_min, mean=mean, scale=scale,
                           clip=(TEC_MIN, TEC_MAX) if self.scaler is not None else None, groups=groups,
                           err_flag=errs.ptr(), outputs=outs)
        if groups is not None:
            errs.post()                        # only a group id can set the word here
        return outs

    def merge_(self, group=None) -> "IntervalMetrics":
        """Sum the statistics over the ranks of `group` with one all-reduce, in place (see `HorizonMetrics.merge_`)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.stats, op=dist.ReduceOp.SUM, group=group)
        return self

    def compute(self) -> Dict[str, object]:
        """The INTERVAL_KEYS as numpy (G, H, N) arrays, NaN where a cell saw no sample; "nominal_coverage" = 1 - alpha;
        "by_group": per group the scores of its statistics pooled over the nodes, by horizon and averaged over the horizons
        (NaN for a group never visited)."""
        st = self.stats.permute(0, 1, 3, 2).cpu().numpy()                   # (G, H, I, 6)
        out: Dict[str, object] = dict(derive_intervals(st))
        out["nominal_coverage"] = self.nominal_coverage
        out["by_group"] = [_pooled_intervals(derive_intervals(st[g].sum(axis=1))) for g in range(self.G)]
        return out


# ------------------------------------------------------------------------------------ quantile forecasts
QUANTILE_LEVEL_KEYS = ("pinball", "reliability")                              # (..., Q)
QUANTILE_PAIR_KEYS = ("interval_width", "coverage", "interval_score")         # (..., P), P = Q // 2
QUANTILE_KEYS = ("count", "crossing_rate", "quantile_crps") + QUANTILE_LEVEL_KEYS + QUANTILE_PAIR_KEYS


def quantile_pairs(taus) -> Tuple[Tuple[float, float, float], ...]:
    """The P = Q // 2 central intervals of the levels: pair r = (tau_r, tau_{Q+1-r}, alpha_r) with the nominal miscoverage
    alpha_r = tau_r + 1 - tau_{Q+1-r}."""
    ts = [float(t) for t in taus]
    return tuple((ts[r], ts[len(ts) - 1 - r], ts[r] + 1.0 - ts[len(ts) - 1 - r]) for r in range(len(ts) // 2))


def crps_weights(taus) -> np.ndarray:
    """Trapezoid weights of the levels in tau: w_q = (tau_{q+1} - tau_{q-1}) / 2 inside, half the neighbouring gap at either
    end; one level alone has the weight 1."""
    ts = np.asarray([float(t) for t in taus], dtype=np.float64)
    if ts.size == 1:
        return np.ones(1)
    w = np.empty_like(ts)
    w[1:-1] = (ts[2:] - ts[:-2]) / 2
    w[0], w[-1] = (ts[1] - ts[0]) / 2, (ts[-1] - ts[-2]) / 2
    return w


def derive_quantiles(stats: np.ndarray, counts: np.ndarray, taus) -> Dict[str, np.ndarray]:
    """(..., 1 + Q + P) float64 sums [count, sum rho_1..Q, sum width_1..P] and integer counts [crossings, hits_1..Q,
    covered_1..P] -> the QUANTILE_KEYS, arrays over the leading axes (a trailing axis of Q or P where named), NaN where a cell
    saw no sample:
      pinball_q = sum rho_q / n, reliability_q = hits_q / n (to be read against tau_q), crossing_rate = crossings / n,
      interval_width_r = sum width_r / n, coverage_r = covered_r / n, and, derived from the pinball means,
      interval_score_r = (2 / alpha_r) (pinball_r + pinball_{Q+1-r})    with alpha_r = tau_r + 1 - tau_{Q+1-r}: the Winkler
                         score of the pair -- for a symmetric pair (tau, 1 - tau) exactly width + (2/alpha) (lo - y)_+ +
                         (2/alpha) (y - hi)_+ averaged over the samples,
      quantile_crps    = 2 sum_q w_q pinball_q    with the trapezoid weights `crps_weights(taus)`: the CRPS integral
                         2 * int_0^1 rho_tau d tau on the levels at hand."""
    ts = [float(t) for t in taus]
    Q, P = len(ts), len(ts) // 2
    st = np.asarray(stats, dtype=np.float64)
    ct = np.asarray(counts).astype(np.float64)
    if st.shape[-1] != 1 + Q + P or ct.shape != st.shape:
        raise ValueError(f"stats and counts must be (..., {1 + Q + P}), got {st.shape} and {ct.shape}")
    n = st[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        nn = n[..., None]
        pin = st[..., 1:1 + Q] / nn
        out = {"count": n.copy(), "crossing_rate": ct[..., 0] / n, "pinball": pin, "reliability": ct[..., 1:1 + Q] / nn,
               "interval_width": st[..., 1 + Q:] / nn, "coverage": ct[..., 1 + Q:] / nn}
        pairs = quantile_pairs(ts)
        out["interval_score"] = np.stack([(2.0 / a) * (pin[..., r] + pin[..., Q - 1 - r]) for r, (_, _, a) in enumerate(pairs)],
                                         axis=-1) if P else np.empty(n.shape + (0,))
        w = crps_weights(ts)
        acc = np.zeros_like(n)
        for q in range(Q):
            acc = acc + w[q] * pin[..., q]
        out["quantile_crps"] = 2.0 * acc
    empty = n == 0
    for k in QUANTILE_KEYS[1:]:
        out[k] = np.where(empty if out[k].ndim == n.ndim else empty[..., None], np.nan, out[k])
    return out


def _pooled_quantiles(per: Dict[str, np.ndarray]) -> Dict[str, object]:
    """`derive_quantiles` of (H, ...) rows -> per key its list by horizon and the average over the horizons."""
    out: Dict[str, object] = {"count_by_horizon": per["count"].tolist()}
    for k in QUANTILE_KEYS[1:]:
        out[f"{k}_by_horizon"] = per[k].tolist()
        out[f"{k}_avg"] = np.mean(per[k], axis=0).tolist() if per[k].ndim > 1 else float(np.mean(per[k]))
    return out


class QuantileMetrics:
    """The scores of a Q-level quantile forecast per cell (group of the sample, horizon, node): per-level pinball loss and
    reliability, the crossing rate, width, coverage and Winkler score of the Q // 2 central intervals, and the quantile CRPS.
    update(levels, true, groups) per batch on the device (one kernel, `tecm_quantile_stats`, no atomics: the same batches
    give the same bits), compute() at the end.  It mirrors `EnsembleMetrics`; the layout convention of the levels is stated
    in include/tecmollm.h (3k)."""

    def __init__(self, num_horizons: int, num_nodes: int, taus, num_groups: int = 1, scaler=None,
                 device: Union[str, torch.device] = "cuda"):
        from tecmollm.functions import quantile_levels
        self.H, self.I, self.G = int(num_horizons), int(num_nodes), int(num_groups)
        if min(self.H, self.I, self.G) < 1:
            raise ValueError("QuantileMetrics needs at least one horizon, one node and one group")
        self.taus = quantile_levels(taus)
        self.Q, self.P = len(self.taus), len(self.taus) // 2
        self.scaler = _scaler_params(scaler)
        rows = 1 + self.Q + self.P
        # [g][h][k][i]: node-contiguous, the layout the kernel's lanes read and write
        self.stats = torch.zeros(self.G, self.H, rows, self.I, device=device, dtype=torch.float64)
        self.counts = torch.zeros(self.G, self.H, rows, self.I, device=device, dtype=torch.int32)

    def reset(self) -> None:
        self.stats.zero_()
        self.counts.zero_()

    def update(self, levels_scaled: torch.Tensor, y_true_scaled: Optional[torch.Tensor], groups: Optional[torch.Tensor] = None,
               adjust: Optional[torch.Tensor] = None, want_sorted: bool = False) -> Optional[torch.Tensor]:
        """levels (S, Q, H, N) in scaled units -- `QuantileModel.quantiles`, read in place whatever its strides --, truth
        (S, H, N) or (S, H, N, 1) or None (nothing is accumulated, only the sorted levels are made); groups (S) int32 or
        None; adjust a contiguous float32 (1 or G, H, Q, N) device tensor added to the sorted levels (`CQRIntervals.on`).
        With `want_sorted` returns the (adjusted) sorted levels in physical units, (S, Q, H, N) float32."""
        from tecmollm import devcheck, ops
        _lib.require_gpu_tensor(levels_scaled, "levels")
        if levels_scaled.dim() != 4 or tuple(levels_scaled.shape[1:]) != (self.Q, self.H, self.I):
            raise ValueError(f"levels must be (S, {self.Q}, {self.H}, {self.I}), got {tuple(levels_scaled.shape)}")
        S = levels_scaled.shape[0]
        truth = None
        if y_true_scaled is not None:
            t, S2, H2, I2, ts, th, ti = _as_shi(y_true_scaled, "y_true")
            if (S2, H2, I2) != (S, self.H, self.I):
                raise ValueError(f"shape mismatch: levels {tuple(levels_scaled.shape)}, y_true {tuple(y_true_scaled.shape)}")
            truth = t.as_strided((S, self.H, self.I), (ts, th, ti))
        if groups is not None:
            _lib.require_gpu_tensor(groups, "groups", torch.int32)
            if groups.shape != (S,):
                raise ValueError(f"groups must hold one id per sample: {tuple(groups.shape)} for {S} samples")
            groups = groups.contiguous()
        mean, scale = self.scaler if self.scaler is not None else (0.0, 1.0)
        errs = devcheck.error_word(self.stats.device)
        out = None
        if want_sorted or truth is None:
            out = torch.empty(S, self.Q, self.H, self.I, device=levels_scaled.device, dtype=torch.float32)
        ops.quantile_stats(levels_scaled.permute(1, 0, 2, 3), truth, self.taus, self.stats, self.counts, adjust=adjust,
                           mean=mean, scale=scale, clip=(TEC_MIN, TEC_MAX) if self.scaler is not None else None,
                           groups=groups, num_groups=self.G, err_flag=errs.ptr(),
                           out_z=out.permute(1, 0, 2, 3) if out is not None else None)
        if groups is not None:
            errs.post()                        # only a group id can set the word here
        return out

    def merge_(self, group=None) -> "QuantileMetrics":
        """Sum the statistics over the ranks of `group` with ONE all-reduce, in place (see `HorizonMetrics.merge_`): the
        counts ride behind the sums as float64 (integers below 2^53: exact)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            both = torch.stack([self.stats, (self.counts.to(torch.int64) & 0xFFFFFFFF).to(torch.float64)])   # unsigned counts
            dist.all_reduce(both, op=dist.ReduceOp.SUM, group=group)
            self.stats.copy_(both[0])
            self.counts.copy_(both[1].to(torch.int64))
        return self

    def compute(self) -> Dict[str, object]:
        """The QUANTILE_KEYS as numpy arrays (G, H, N), with a trailing axis of Q for `pinball` and `reliability` and of
        P = Q // 2 for `interval_width`, `coverage` and `interval_score` (`derive_quantiles` states the formulas), NaN where a
        cell saw no sample; "taus"; "pairs": per central interval (tau_lo, tau_hi, alpha); "by_group": per group the scores
        of its statistics pooled over the nodes, by horizon and averaged over the horizons."""
        st = self.stats.permute(0, 1, 3, 2).cpu().numpy()                   # (G, H, I, 1 + Q + P)
        ct = self.counts.permute(0, 1, 3, 2).cpu().numpy().astype(np.int64)
        if self.counts.dtype == torch.int32:
            ct &= 0xFFFFFFFF                                                # the kernel counts unsigned
        out: Dict[str, object] = dict(derive_quantiles(st, ct, self.taus))
        out["taus"] = list(self.taus)
        out["pairs"] = [list(p) for p in quantile_pairs(self.taus)]
        out["by_group"] = [_pooled_quantiles(derive_quantiles(st[g].sum(axis=1), ct[g].sum(axis=1), self.taus))
                           for g in range(self.G)]
        return out


# ------------------------------------------------------------------------------------ event verification
EVENT_CATEGORICAL_KEYS = ("base_rate", "pod", "far", "pofd", "csi", "ets", "hss", "frequency_bias")
EVENT_PROBABILISTIC_KEYS = ("brier", "brier_reliability", "brier_resolution", "brier_uncertainty", "brier_skill", "roc_area")
EVENT_KEYS = EVENT_CATEGORICAL_KEYS + EVENT_PROBABILISTIC_KEYS
EVENT_TABLE = ("hits", "false_alarms", "misses", "correct_negatives")


def _categorical(a, b, c, d) -> Dict[str, np.ndarray]:
    """The EVENT_CATEGORICAL_KEYS of float64 tables [hits a, false alarms b, misses c, correct negatives d] of any shape,
    NaN where a denominator is 0: base_rate (a+c)/n, pod a/(a+c), far b/(a+b) (the false-alarm RATIO), pofd b/(b+d), csi
    a/(a+b+c), ets (a-r)/(a+b+c-r) with r = (a+b)(a+c)/n, hss 2(ad-bc)/((a+c)(c+d)+(a+b)(b+d)), frequency_bias (a+b)/(a+c)."""
    n = a + b + c + d
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (a + b) * (a + c) / n
        return {"base_rate": (a + c) / n, "pod": a / (a + c), "far": b / (a + b), "pofd": b / (b + d),
                "csi": a / (a + b + c), "ets": (a - r) / (a + b + c - r),
                "hss": 2.0 * (a * d - b * c) / ((a + c) * (c + d) + (a + b) * (b + d)),
                "frequency_bias": (a + b) / (a + c)}


def _probabilistic(n: np.ndarray, o: np.ndarray) -> Dict[str, np.ndarray]:
    """Float64 counts n_j, o_j of shape (..., K+1) -> the EVENT_PROBABILISTIC_KEYS over the leading axes plus "roc_curve"
    (..., K+2, 2) = (pofd, pod) from (0, 0) to (1, 1).  The forecast probability of count j is j / K."""
    K = n.shape[-1] - 1
    f = np.arange(K + 1, dtype=np.float64) / K
    with np.errstate(divide="ignore", invalid="ignore"):
        N = n.sum(axis=-1)
        obar = o.sum(axis=-1) / N
        bs = ((n - o) * f * f + o * (1.0 - f) * (1.0 - f)).sum(axis=-1) / N
        oj = np.where(n > 0, o / np.where(n > 0, n, 1.0), 0.0)               # an empty bin adds nothing to either term
        rel = (n * (f - oj) ** 2).sum(axis=-1) / N
        res = (n * (oj - obar[..., None]) ** 2).sum(axis=-1) / N
        unc = obar * (1.0 - obar)
        skill = 1.0 - bs / unc
        # "at least j members", j = K+1 (never), K, ..., 1, 0 (always)
        ev, ne = o.sum(axis=-1, keepdims=True), (n - o).sum(axis=-1, keepdims=True)
        zero = np.zeros(n.shape[:-1] + (1,))
        hit = np.concatenate([zero, np.cumsum(o[..., ::-1], axis=-1)], axis=-1) / ev
        fa = np.concatenate([zero, np.cumsum((n - o)[..., ::-1], axis=-1)], axis=-1) / ne
        area = (0.5 * (hit[..., 1:] + hit[..., :-1]) * (fa[..., 1:] - fa[..., :-1])).sum(axis=-1)
    return {"brier": bs, "brier_reliability": rel, "brier_resolution": res, "brier_uncertainty": unc, "brier_skill": skill,
            "roc_area": area, "roc_curve": np.stack([fa, hit], axis=-1)}


def derive_events(hist: np.ndarray) -> Dict[str, np.ndarray]:
    """(G, Q, H, K+1, 2, N) integer counts of `tecm_event_hist` -- [..., j, 0, i] the samples in which exactly j members
    forecast the event, [..., j, 1, i] those of them in which it occurred -- -> float64 scores, NaN where a denominator is 0:
      "count" (G, Q, H, N), "table" (G, Q, H, 4, N) = EVENT_TABLE, where the forecast says yes when at least half the members
      do (2 j >= K; for K = 1 the forecast itself: o_1 hits, n_1 - o_1 false alarms, o_0 misses, n_0 - o_0 correct negatives);
      the EVENT_CATEGORICAL_KEYS as (G, Q, H, N), as "<key>_pooled" (G, Q, H) from the tables summed over the nodes and as
      "<key>_all" (G, Q) from the tables summed over nodes and horizons (summed tables, not averaged ratios), with
      "table_pooled" (G, Q, H, 4) and "table_all" (G, Q, 4);
      for K > 1 the EVENT_PROBABILISTIC_KEYS in the same three forms -- Brier score, its reliability / resolution /
      uncertainty terms (forecasts take the K + 1 values j / K, so BS = REL - RES + UNC holds exactly), the skill against
      the sample's own base rate, the area under the ROC (trapezoid over the K + 2 points "at least j members", (0, 0) and
      (1, 1) included) -- plus "reliability" (G, Q, H, K+1, 2) = (n_j, o_j / n_j) and "roc_curve" (G, Q, H, K+2, 2) = (pofd,
      pod), both pooled over the nodes."""
    hs = np.asarray(hist)
    if hs.ndim != 6 or hs.shape[4] != 2 or not np.issubdtype(hs.dtype, np.integer):
        raise ValueError(f"hist must be an integer (G, Q, H, K+1, 2, N) array, got {hs.dtype} {hs.shape}")
    hs = hs.astype(np.int64)
    K = hs.shape[3] - 1
    n_j, o_j = hs[:, :, :, :, 0, :], hs[:, :, :, :, 1, :]                  # (G, Q, H, K+1, N)
    yes = 2 * np.arange(K + 1) >= K
    a, c = o_j[:, :, :, yes].sum(axis=3), o_j[:, :, :, ~yes].sum(axis=3)
    b, d = n_j[:, :, :, yes].sum(axis=3) - a, n_j[:, :, :, ~yes].sum(axis=3) - c
    table = np.stack([a, b, c, d], axis=3)                                 # (G, Q, H, 4, N) int64
    out: Dict[str, np.ndarray] = {"count": n_j.sum(axis=3).astype(np.float64), "table": table.astype(np.float64)}
    forms = (("", table), ("_pooled", table.sum(axis=4)), ("_all", table.sum(axis=(2, 4))))
    for suffix, t in forms:
        if suffix:
            out["table" + suffix] = t.astype(np.float64)
        axis = 3 if suffix != "_all" else 2
        parts = [np.take(t, k, axis=axis).astype(np.float64) for k in range(4)]
        for k, v in _categorical(*parts).items():
            out[k + suffix] = v
    if K > 1:
        no = np.stack([n_j, o_j], axis=-1)                                 # (G, Q, H, K+1, N, 2)
        per_node = np.moveaxis(no, 3, 4)                                   # (G, Q, H, N, K+1, 2)
        pooled, everything = no.sum(axis=4), no.sum(axis=(2, 4))           # (G, Q, H, K+1, 2), (G, Q, K+1, 2)
        for suffix, t in (("", per_node), ("_pooled", pooled), ("_all", everything)):
            t = t.astype(np.float64)
            prob = _probabilistic(t[..., 0], t[..., 1])
            for k in EVENT_PROBABILISTIC_KEYS:
                out[k + suffix] = prob[k]
            if suffix == "_pooled":
                out["roc_curve"] = prob["roc_curve"]
        with np.errstate(divide="ignore", invalid="ignore"):
            n, o = pooled[..., 0].astype(np.float64), pooled[..., 1].astype(np.float64)
            out["reliability"] = np.stack([n, o / n], axis=-1)
    return out


def derive_fss(sums: np.ndarray, base_rate: np.ndarray) -> Dict[str, np.ndarray]:
    """(G, Q, H, W, 3) integer sums [sum (cf - co)^2, sum cf^2, sum co^2] of `tecm_event_fss` -> "fss" (G, Q, H, W) = 1 -
    sums[0] / (sums[1] + sums[2]), NaN where neither field ever held an event; "fss_pooled" (G, Q, W) from the sums added over
    the horizons; "fss_uniform" = 0.5 + f_o / 2 with f_o = `base_rate` (any shape): the score of a forecast as large as the
    observed fraction everywhere, above which a scale counts as skilful (Roberts & Lean 2008)."""
    sm = np.asarray(sums)
    if sm.ndim != 5 or sm.shape[-1] != 3:
        raise ValueError(f"sums must be (G, Q, H, W, 3), got {sm.shape}")
    sm = sm.astype(np.float64)
    tot = sm.sum(axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"fss": 1.0 - sm[..., 0] / (sm[..., 1] + sm[..., 2]),
                "fss_pooled": 1.0 - tot[..., 0] / (tot[..., 1] + tot[..., 2]),
                "fss_uniform": 0.5 + np.asarray(base_rate, dtype=np.float64) / 2.0}


class EventMetrics:
    """Event verification per cell (group of the sample, threshold, horizon, node): did the forecast announce that TEC would
    cross a threshold?  `thresholds` is a `tecmollm.events.EventThresholds`.  update(pred_or_members, true, groups, slots) per
    batch on the device (`tecm_event_hist`, and with `grid` = (rows, cols) `tecm_event_fss` over the window widths `scales`):
    integer counts only, so the same batches in any order give the same bits.  members = 1 scores a deterministic forecast
    (contingency scores, FSS), members = K > 1 an ensemble (Brier score and its decomposition, reliability, ROC), compute()
    at the end."""

    def __init__(self, num_horizons: int, num_nodes: int, thresholds, num_groups: int = 1, scaler=None, members: int = 1,
                 grid=None, scales=(1, 3, 5, 9), device: Union[str, torch.device] = "cuda"):
        self.H, self.I, self.G, self.K = int(num_horizons), int(num_nodes), int(num_groups), int(members)
        if min(self.H, self.I, self.G) < 1:
            raise ValueError("EventMetrics needs at least one horizon, one node and one group")
        if not 1 <= self.K <= _lib.TECM_ENS_MAX_K:
            raise ValueError(f"members must lie in [1, {_lib.TECM_ENS_MAX_K}], got {self.K}")
        self.thresholds = thresholds
        self.Q = thresholds.Q
        if not 1 <= self.Q <= _lib.TECM_EVENT_MAX_Q:
            raise ValueError(f"between 1 and {_lib.TECM_EVENT_MAX_Q} thresholds, got {self.Q}")
        if thresholds.num_nodes not in (None, self.I):
            raise ValueError(f"the thresholds hold {thresholds.num_nodes} nodes, the forecast {self.I}")
        self.scaler = _scaler_params(scaler)
        self.thr = thresholds.tensor(device)
        # [g][q][h][j][e][i]: node-contiguous, the layout the kernel's lanes read and write
        self.hist = torch.zeros(self.G, self.Q, self.H, self.K + 1, 2, self.I, device=device, dtype=torch.int32)
        self.grid, self.scales, self.sums = None, tuple(int(w) for w in scales), None
        if grid is not None:
            from tecmollm import ops
            if self.K != 1:
                raise ValueError("the FSS is taken of a deterministic forecast: grid needs members = 1")
            self.grid = (int(grid[0]), int(grid[1]))
            if self.grid[0] * self.grid[1] != self.I:
                raise ValueError(f"grid {self.grid} does not hold {self.I} nodes")
            if not 1 <= len(self.scales) <= _lib.TECM_EVENT_MAX_W or any(w < 1 or w > 127 or w % 2 == 0 for w in self.scales):
                raise ValueError(f"scales must be 1 to {_lib.TECM_EVENT_MAX_W} odd widths in [1, 127], got {self.scales}")
            if not ops.event_fss_ok(*self.grid):
                raise TecmError(f"tecm_event_fss does not serve a {self.grid[0]} x {self.grid[1]} grid (its tables exceed 64 KiB of LDS)")
            self.sums = torch.zeros(self.G, self.Q, self.H, len(self.scales), 3, device=device, dtype=torch.int64)

    def reset(self) -> None:
        self.hist.zero_()
        if self.sums is not None:
            self.sums.zero_()

    def update(self, pred_or_members: torch.Tensor, y_true_scaled: torch.Tensor, groups: Optional[torch.Tensor] = None,
               slots: Optional[torch.Tensor] = None) -> None:
        """members = 1: the forecast (S, H, N) or (S, H, N, 1); members = K > 1: (K, S, H, N) or (K, S, H, N, 1); the truth
        (S, H, N) or (S, H, N, 1); all in scaled units and read in place whatever their strides.  groups (S) int32 or None;
        slots (S, H) int32, the time-of-day slot of every target step (`tecmollm.events.target_slots`), needed exactly when
        the thresholds depend on the slot."""
        from tecmollm import devcheck, ops
        t, S, H, I, ts, th, ti = _as_shi(y_true_scaled, "y_true")
        if self.K == 1:
            p, S2, H2, I2, ps, ph, pi = _as_shi(pred_or_members, "y_pred")
            m = p.as_strided((1, S2, H2, I2), (0, ps, ph, pi))
        else:
            m = pred_or_members
            _lib.require_gpu_tensor(m, "members")
            if m.dim() == 5 and m.shape[-1] == 1:
                m = m.squeeze(-1)
            if m.dim() != 4:
                raise ValueError(f"members must be (K, S, H, N), got {tuple(pred_or_members.shape)}")
        if tuple(m.shape) != (self.K, S, H, I) or H != self.H or I != self.I:
            raise ValueError(f"shape mismatch: forecast {tuple(pred_or_members.shape)}, true {tuple(y_true_scaled.shape)}, "
                             f"expected members {self.K}, horizons {self.H}, nodes {self.I}")
        if groups is not None:
            _lib.require_gpu_tensor(groups, "groups", torch.int32)
            if groups.shape != (S,):
                raise ValueError(f"groups must hold one id per sample: {tuple(groups.shape)} for {S} samples")
            groups = groups.contiguous()
        num_slots = self.thresholds.num_slots
        if (slots is None) != (num_slots == 1):
            raise ValueError("slots are needed exactly when the thresholds depend on the time-of-day slot")
        if slots is not None:
            _lib.require_gpu_tensor(slots, "slots", torch.int32)
            if slots.shape != (S, H):
                raise ValueError(f"slots must be (S, H) = {(S, H)}, got {tuple(slots.shape)}")
            slots = slots.contiguous()
        mean, scale = self.scaler if self.scaler is not None else (0.0, 1.0)
        errs = devcheck.error_word(self.hist.device)
        target = t.as_strided((S, H, I), (ts, th, ti))
        common = dict(slots=slots, num_slots=num_slots, mean=mean, scale=scale,
                      clip=(TEC_MIN, TEC_MAX) if self.scaler is not None else None, groups=groups, err_flag=errs.ptr())
        ops.event_hist(m, target, self.hist, self.thr, self.thresholds.strides, self.thresholds.dirs, **common)
        if self.sums is not None:
            ops.event_fss(m[0], target, self.sums, self.thr, self.thresholds.strides, self.thresholds.dirs, self.scales,
                          self.grid, **common)
        if groups is not None or slots is not None:
            errs.post()                        # only a group or slot id can set the word here

    def merge_(self, group=None) -> "EventMetrics":
        """Sum the counts (and the FSS sums) over the ranks of `group`, in place: all of them live in one int64 buffer for
        the length of ONE all-reduce.  See `HorizonMetrics.merge_`."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            n = self.hist.numel()
            parts = [self.hist.reshape(-1).to(torch.int64)] + ([self.sums.reshape(-1)] if self.sums is not None else [])
            flat = torch.cat(parts)
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
            self.hist.copy_(flat[:n].view_as(self.hist).to(torch.int32))
            if self.sums is not None:
                self.sums.copy_(flat[n:].view_as(self.sums))
        return self

    def compute(self) -> Dict[str, object]:
        """`derive_events` of the counts (and `derive_fss` of the sums, with the pooled base rate), plus "thresholds" (the
        labels), "members" and, with a grid, "scales"."""
        out: Dict[str, object] = dict(derive_events(self.hist.cpu().numpy().astype(np.int64)))
        if self.sums is not None:
            out.update(derive_fss(self.sums.cpu().numpy(), out["base_rate_pooled"]))
            out["scales"] = list(self.scales)
        out["thresholds"] = list(self.thresholds.labels)
        out["members"] = self.K
        return out


# ------------------------------------------------------------------------------------ multivariate (field) scores
FIELD_KEYS = ("count", "energy_score", "fair_energy_score", "field_error_mean", "pairs", "variogram_score",
              "variogram_score_per_pair", "variogram_obs", "variogram_ens", "variogram_ratio")


def derive_fields(es_stats: np.ndarray, vs_stats: np.ndarray, members: int) -> Dict[str, np.ndarray]:
    """(..., 4) float64 sums [n, sum A, sum D, sum E] and (..., NB, 5) sums [n, sum pairs, sum e^2, sum v_o, sum v_e] (NB may
    be 0) -> the FIELD_KEYS, NaN where nothing was seen:
      energy_score = mean(A) - mean(D) / K^2        fair_energy_score = mean(A) - mean(D) / (K (K - 1))   (NaN for K = 1)
      field_error_mean = mean(E), the Euclidean error of the ensemble-mean map (K = 1: equal to the energy score)
      variogram_score = (sum e^2) / n, the score of a class per window     variogram_score_per_pair = (sum e^2) / pairs
      variogram_obs, variogram_ens = (sum v_o) / pairs, (sum v_e) / pairs   variogram_ratio = variogram_ens / variogram_obs
    (a ratio below 1: the members are smoother than the truth at that distance; above 1: rougher.)  "count" is n (...),
    "pairs" the number of pairs counted (..., NB), over all windows."""
    K = int(members)
    es = np.asarray(es_stats, dtype=np.float64)
    vs = np.asarray(vs_stats, dtype=np.float64)
    if K < 1 or es.shape[-1] != _lib.TECM_FIELD_ES_STATS or vs.shape[-1] != _lib.TECM_FIELD_VS_STATS or vs.shape[:-2] != es.shape[:-1]:
        raise ValueError(f"es_stats (..., 4) and vs_stats (..., NB, 5) do not fit (members {K}): {es.shape}, {vs.shape}")
    n, sA, sD, sE = np.moveaxis(es, -1, 0)
    nv, sp, se2, svo, sve = np.moveaxis(vs, -1, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        fair = (sA - sD / (K * (K - 1))) / n if K > 1 else np.full_like(n, np.nan)
        out = {"count": n.copy(), "energy_score": (sA - sD / (K * K)) / n, "fair_energy_score": fair,
               "field_error_mean": sE / n, "pairs": sp.copy(), "variogram_score": se2 / nv,
               "variogram_score_per_pair": se2 / sp, "variogram_obs": svo / sp, "variogram_ens": sve / sp,
               "variogram_ratio": sve / svo}
    for k in ("energy_score", "fair_energy_score", "field_error_mean"):
        out[k] = np.where(n == 0, np.nan, out[k])
    out["variogram_score"] = np.where(nv == 0, np.nan, out["variogram_score"])
    for k in ("variogram_score_per_pair", "variogram_obs", "variogram_ens", "variogram_ratio"):
        out[k] = np.where(sp == 0, np.nan, out[k])
    return out


class FieldMetrics:
    """Multivariate scores of a K-member ensemble per (group of the sample, horizon): the energy score and, with a class
    matrix (`tecmollm.fields.pair_classes`), the variogram score of order 0.5, 1 or 2 per class of node pairs -- the scores
    that see whether a member is a plausible map, which `EnsembleMetrics` cannot (it sorts the members of every cell).
    update(members, true, groups) per batch on the device (`tecm_field_scores`: no host copy of the members, no atomics on
    the sums, so the same batches give the same bits), compute() at the end.  members = 1 scores a point forecast's map."""

    def __init__(self, num_horizons: int, num_nodes: int, members: int, pair_class: Optional[torch.Tensor] = None,
                 num_classes: int = 0, order: float = 0.5, num_groups: int = 1, scaler=None,
                 device: Union[str, torch.device] = "cuda"):
        from tecmollm import ops
        self.H, self.I, self.K, self.G, self.NB = int(num_horizons), int(num_nodes), int(members), int(num_groups), int(num_classes)
        if min(self.H, self.I, self.G) < 1:
            raise ValueError("FieldMetrics needs at least one horizon, one node and one group")
        if not 1 <= self.K <= _lib.TECM_ENS_MAX_K:
            raise ValueError(f"members must lie in [1, {_lib.TECM_ENS_MAX_K}], got {self.K}")
        if not 0 <= self.NB <= _lib.TECM_FIELD_MAX_CLASSES:
            raise ValueError(f"num_classes must lie in [0, {_lib.TECM_FIELD_MAX_CLASSES}], got {self.NB}")
        if float(order) not in ops.FIELD_ORDERS:
            raise ValueError(f"order must be one of {sorted(ops.FIELD_ORDERS)}, got {order}")
        if (pair_class is None) != (self.NB == 0):
            raise ValueError("pair_class and num_classes > 0 go together")
        self.order = float(order)
        self.pair_class = None
        if pair_class is not None:
            pc = torch.as_tensor(pair_class)
            if pc.dtype != torch.uint8 or pc.shape != (self.I, self.I):
                raise ValueError(f"pair_class must be a uint8 ({self.I}, {self.I}) matrix, got {pc.dtype} {tuple(pc.shape)}")
            self.pair_class = pc.to(device).contiguous()
        self.scaler = _scaler_params(scaler)
        self.es_stats = torch.zeros(self.G, self.H, _lib.TECM_FIELD_ES_STATS, device=device, dtype=torch.float64)
        self.vs_stats = torch.zeros(self.G, self.H, self.NB, _lib.TECM_FIELD_VS_STATS, device=device, dtype=torch.float64)
        self._ws: Optional[torch.Tensor] = None

    def reset(self) -> None:
        self.es_stats.zero_()
        self.vs_stats.zero_()

    def update(self, members_scaled: torch.Tensor, y_true_scaled: torch.Tensor, groups: Optional[torch.Tensor] = None,
               outputs=()) -> Dict[str, torch.Tensor]:
        """members (K, S, H, N) or (K, S, H, N, 1) -- for members = 1 also a forecast (S, H, N[, 1]) -- and the truth (S, H, N)
        or (S, H, N, 1), in scaled units and read in place whatever their strides; groups (S) int32 or None.  Returns the
        per-sample tensors named in `outputs`, float64: "energy" (S, H, 3) = [A, D, E] and "variogram" (S, H, NB, 4) =
        [pairs, sum e^2, sum v_o, sum v_e]; the rows of a sample with a bad group id are NaN."""
        from tecmollm import devcheck, ops
        t, S, H, I, ts, th, ti = _as_shi(y_true_scaled, "y_true")
        m = members_scaled
        _lib.require_gpu_tensor(m, "members")
        if m.dim() == 5 and m.shape[-1] == 1:
            m = m.squeeze(-1)
        if self.K == 1 and m.dim() in (3, 4) and tuple(m.shape) != (1, S, H, I) and tuple(m.shape[:2]) == (S, H):
            p, S2, H2, I2, ps, ph, pi = _as_shi(members_scaled, "y_pred")
            m = p.as_strided((1, S2, H2, I2), (0, ps, ph, pi))
        if m.dim() != 4:
            raise ValueError(f"members must be (K, S, H, N), got {tuple(members_scaled.shape)}")
        if tuple(m.shape) != (self.K, S, H, I) or H != self.H or I != self.I:
            raise ValueError(f"shape mismatch: members {tuple(members_scaled.shape)}, true {tuple(y_true_scaled.shape)}, "
                             f"expected members {self.K}, horizons {self.H}, nodes {self.I}")
        if groups is not None:
            _lib.require_gpu_tensor(groups, "groups", torch.int32)
            if groups.shape != (S,):
                raise ValueError(f"groups must hold one id per sample: {tuple(groups.shape)} for {S} samples")
            groups = groups.contiguous()
        unknown = set(outputs) - {"energy", "variogram"}
        if unknown:
            raise ValueError(f"outputs must come from ('energy', 'variogram'), got {sorted(unknown)}")
        outs: Dict[str, torch.Tensor] = {}
        if "energy" in outputs:
            outs["energy"] = torch.full((S, H, 3), float("nan"), device=m.device, dtype=torch.float64)
        if "variogram" in outputs:
            outs["variogram"] = torch.full((S, H, self.NB, 4), float("nan"), device=m.device, dtype=torch.float64)
        mean, scale = self.scaler if self.scaler is not None else (0.0, 1.0)
        errs = devcheck.error_word(self.es_stats.device)
        self._ws = ops.field_scores(m, t.as_strided((S, H, I), (ts, th, ti)), self.es_stats, self.vs_stats, self.pair_class,
                                    order=self.order, mean=mean, scale=scale,
                                    clip=(TEC_MIN, TEC_MAX) if self.scaler is not None else None, groups=groups,
                                    err_flag=errs.ptr(), es_out=outs.get("energy"), vs_out=outs.get("variogram"),
                                    workspace=self._ws)
        if groups is not None:
            errs.post()                        # only a group id can set the word here
        return outs

    def merge_(self, group=None) -> "FieldMetrics":
        """Sum both statistics over the ranks of `group`, in place: they live in one buffer for the length of ONE
        all-reduce.  See `HorizonMetrics.merge_`."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            n = self.es_stats.numel()
            flat = torch.cat([self.es_stats.reshape(-1), self.vs_stats.reshape(-1)])
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
            self.es_stats.copy_(flat[:n].view_as(self.es_stats))
            self.vs_stats.copy_(flat[n:].view_as(self.vs_stats))
        return self

    def compute(self) -> Dict[str, object]:
        """`derive_fields` of the statistics: the FIELD_KEYS as numpy arrays, (G, H) for the energy score and the count,
        (G, H, NB) for the variogram keys and the pair counts; NaN where nothing was seen."""
        return dict(derive_fields(self.es_stats.cpu().numpy(), self.vs_stats.cpu().numpy(), self.K))
