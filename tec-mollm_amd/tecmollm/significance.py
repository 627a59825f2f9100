"""Is the difference larger than the noise of the split?  Block-bootstrap intervals and Diebold-Mariano tests.

`evaluate_split` ends in one comparison -- `improvement()`'s four percentages -- and says nothing about its uncertainty.
The windows of a split overlap (stride-1 windows share all but one input and target row), so their errors are strongly
autocorrelated and a standard error that treats them as independent is several times too small.  Two standard answers:

  * the circular block bootstrap of the WINDOWS: resample blocks of consecutive windows, the same blocks for every forecast
    (paired), and recompute every metric and the improvement percentages per replicate -> percentile intervals;
  * the Diebold-Mariano test on the per-window loss differential with a Bartlett (Newey-West) long-run variance and the
    Harvey-Leybourne-Newbold small-sample factor -> "is forecast A's loss lower than forecast B's".

Both need the statistics of every window kept apart, which `HorizonMetrics` (pooled with atomics) and `MapMetrics` (per
node) do not keep:

  * `WindowScores` holds the (forecasts, windows, horizons, 8) float64 table on the device; `update` writes the rows of a
    batch (`tecm_metrics_window`: the eight sums of `HorizonMetrics` per (window, horizon), fixed order, no atomics);
  * `block_bootstrap` resamples it there (`tecm_block_bootstrap`: ordered float64 sums, bit-reproducible);
  * `bootstrap_intervals` and `diebold_mariano` finish on the host in float64 numpy: a few thousand numbers.

Not covered: automatic block-length selection, studentised / BCa intervals, per-node tables, the ensemble and conformal
statistics (the bootstrap kernel takes any row width, so they can follow).
"""
from __future__ import annotations

import csv
import ctypes as C
import math
import os
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import TecmBlockBootstrap, TecmMetricsWindow, check, lib, stream_ptr
from .devcheck import check_device_errors, error_word
from .evaluate import MODEL_NAME, _score_pass, baseline_name

TEC_MIN, TEC_MAX = 0.0, 200.0
STATS = _lib.TECM_METRIC_STATS
AVERAGES = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg")
IMPROVEMENTS = ("mae", "rmse", "r2_score", "pearson_r")
LOSSES = {"se": 7, "ae": 6}                 # column of the table: sum (t-p)^2, sum |t-p|


# ------------------------------------------------------------------------------------------------ the two launches
def window_stats(pred: torch.Tensor, true: torch.Tensor, table: torch.Tensor, rows: Optional[torch.Tensor] = None,
                 row0: int = 0, scaler: Optional[Tuple[float, float]] = None) -> None:
    """`tecm_metrics_window`: write the (H, 8) statistics of every sample of `pred` / `true` ((S, H, N[, 1]) float32 on the
    device, scaled units, read in place) into row `rows[s]` (int64 on the device) or `row0 + s` of `table`
    ((rows, H, 8) float64, contiguous).  A row outside the table writes nothing and raises `TecmError` at the next
    `check_device_errors`."""
    from src.evaluation.metrics import _as_shi
    p, S, H, I, ps, ph, pi = _as_shi(pred, "y_pred")
    t, S2, H2, I2, ts, th, ti = _as_shi(true, "y_true")
    _lib.require_gpu_tensor(table, "table", torch.float64)
    if (S, H, I) != (S2, H2, I2) or table.dim() != 3 or tuple(table.shape[1:]) != (H, STATS) or not table.is_contiguous():
        raise ValueError(f"shape mismatch: pred {tuple(pred.shape)}, true {tuple(true.shape)}, table {tuple(table.shape)}")
    if rows is not None:
        _lib.require_gpu_tensor(rows, "rows", torch.int64)
        if rows.shape != (S,):
            raise ValueError(f"rows must hold one index per sample: {tuple(rows.shape)} for {S} samples")
        rows = rows.contiguous()
    mean, scale = scaler if scaler is not None else (0.0, 1.0)
    errs = error_word(table.device)
    m = TecmMetricsWindow(pred=p.data_ptr(), p_stride_s=ps, p_stride_h=ph, p_stride_i=pi,
                          target=t.data_ptr(), t_stride_s=ts, t_stride_h=th, t_stride_i=ti,
                          S=S, H=H, I=I, mean=mean, scale=scale, clip_lo=TEC_MIN, clip_hi=TEC_MAX,
                          clip=1 if scaler is not None else 0, table=table.data_ptr(), table_rows=table.shape[0],
                          rows=_lib.ptr(rows), row0=int(row0), err_flag=errs.ptr())
    check(lib().tecm_metrics_window(C.byref(m), stream_ptr()), "tecm_metrics_window")
    errs.post()


def bootstrap_sums(table: torch.Tensor, starts: torch.Tensor, block_len: int, groups: Optional[torch.Tensor] = None,
                   num_groups: int = 1) -> torch.Tensor:
    """`tecm_block_bootstrap`: `table` (M, S, W) float64 on the device (last axis contiguous), `starts` (R, K) int32 with
    K = ceil(S / block_len), `groups` (S) int32 in [0, num_groups) or None -> (R, M, G, W) float64: per replicate the
    sum, in resampled order, of the rows of every group.  A start outside [0, S) or a group id outside its range skips
    its windows and raises `TecmError` at the next `check_device_errors`."""
    _lib.require_gpu_tensor(table, "table", torch.float64)
    _lib.require_gpu_tensor(starts, "starts", torch.int32)
    if table.dim() != 3 or starts.dim() != 2:
        raise ValueError(f"table must be (M, S, W) and starts (R, K), got {tuple(table.shape)} and {tuple(starts.shape)}")
    M, S, W = table.shape
    if W > 1 and table.stride(2) != 1:
        table = table.contiguous()
    starts = starts.contiguous()
    R, K = starts.shape
    G = int(num_groups)
    if groups is not None:
        _lib.require_gpu_tensor(groups, "groups", torch.int32)
        if groups.shape != (S,):
            raise ValueError(f"groups must hold one id per window: {tuple(groups.shape)} for {S} windows")
        groups = groups.contiguous()
    if min(M, S, W, R, G) < 1:
        raise ValueError("block bootstrap of an empty table")
    out = torch.empty(R, M, G, W, device=table.device, dtype=torch.float64)
    errs = error_word(table.device)
    b = TecmBlockBootstrap(table=table.data_ptr(), stride_m=table.stride(0) if M > 1 else 0,
                           stride_s=table.stride(1) if S > 1 else W, M=M, S=S, W=W, group=_lib.ptr(groups), G=G,
                           starts=starts.data_ptr(), R=R, K=K, L=int(block_len), out=out.data_ptr(), err_flag=errs.ptr())
    check(lib().tecm_block_bootstrap(C.byref(b), stream_ptr()), "tecm_block_bootstrap")
    errs.post()
    return out


# ------------------------------------------------------------------------------------------------ host arithmetic
def bootstrap_rows(starts: Sequence[int], num_windows: int, block_len: int) -> List[int]:
    """The windows one replicate visits, in order: position t = k*L + j reads window (starts[k] + j) mod S; the last block
    is truncated so that exactly S windows are read.  Needs len(starts) == ceil(S / L)."""
    S, L = int(num_windows), int(block_len)
    if S < 1 or L < 1 or len(starts) != -(-S // L):
        raise ValueError(f"need S >= 1, L >= 1 and ceil(S / L) = {-(-S // L) if S > 0 and L > 0 else '?'} starts, got {len(starts)}")
    return [(int(starts[t // L]) + t % L) % S for t in range(S)]


def draw_starts(num_windows: int, block_len: int, replicates: int, seed: int) -> torch.Tensor:
    """(R, ceil(S / L)) int32 block starts, uniform on [0, S), from a seeded CPU generator: the same on every machine."""
    S, L, R = int(num_windows), int(block_len), int(replicates)
    if S < 1 or L < 1 or R < 1:
        raise ValueError("need at least one window, one replicate and block_len >= 1")
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    return torch.randint(0, S, (R, -(-S // L)), generator=gen, dtype=torch.int32)


def default_block_len(num_windows: int, L_in: int, L_out: int, stride: int = 1) -> int:
    """min(2 * ceil((L_in + L_out) / stride), max(1, S // 8)): twice the span over which two windows share data, capped
    so that at least eight blocks are drawn.  A rule of thumb, not an estimate."""
    return min(2 * -(-(int(L_in) + int(L_out)) // int(stride)), max(1, int(num_windows) // 8))


def default_lags(num_windows: int, L_out: int, stride: int = 1) -> int:
    """max(ceil(L_out / stride) - 1, floor(4 (S / 100)^(2/9))): the lags over which two windows share target rows, or the
    Newey-West rule, whichever is larger."""
    return max(-(-int(L_out) // int(stride)) - 1, int(math.floor(4.0 * (int(num_windows) / 100.0) ** (2.0 / 9.0))))


def interval_ranks(count: int, level) -> Tuple[int, int]:
    """The 0-based ranks, among `count` sorted values, of the ends of the percentile interval at `level`, rounded outward:
    floor((alpha / 2)(R - 1)) and ceil((1 - alpha / 2)(R - 1)) with alpha = 1 - level, in exact rational arithmetic on the
    decimal `level` as written."""
    R = int(count)
    lv = level if isinstance(level, Fraction) else Fraction(str(level))
    if not 0 < lv < 1:
        raise ValueError(f"level must lie in (0, 1), got {level}")
    if R < 1:
        raise ValueError("no value to rank")
    half = (1 - lv) / 2
    return math.floor(half * (R - 1)), math.ceil((1 - half) * (R - 1))


def percentile_interval(values: np.ndarray, level) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(R, ...) replicate values -> (lo, hi, nan_count) over the leading axis: order statistics at `interval_ranks` of the
    values that are not NaN, no interpolation.  NaN replicates are counted, not ranked; a column of NaNs only gives NaN."""
    v = np.sort(np.asarray(values, dtype=np.float64), axis=0)                # NaN sorts last
    nan = np.isnan(v).sum(axis=0)
    valid = v.shape[0] - nan
    lo_rank, hi_rank = np.zeros(valid.shape, dtype=np.int64), np.zeros(valid.shape, dtype=np.int64)
    for n in np.unique(valid):
        if n > 0:
            lo_rank[valid == n], hi_rank[valid == n] = interval_ranks(int(n), level)
    lo = np.take_along_axis(v, lo_rank[None], axis=0)[0]
    hi = np.take_along_axis(v, hi_rank[None], axis=0)[0]
    return np.where(valid > 0, lo, np.nan), np.where(valid > 0, hi, np.nan), nan


def _betacf(a: float, b: float, x: float) -> float:
    """The continued fraction of the incomplete beta function (modified Lentz)."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 100000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h


def betainc(a: float, b: float, x: float) -> float:
    """The regularised incomplete beta function I_x(a, b), a, b > 0, 0 <= x <= 1; pure Python."""
    if not (a > 0 and b > 0) or not 0.0 <= x <= 1.0:
        raise ValueError(f"betainc needs a, b > 0 and 0 <= x <= 1, got {a}, {b}, {x}")
    if x == 0.0 or x == 1.0:
        return x
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _betacf(a, b, x) / a
    return 1.0 - front * _betacf(b, a, 1.0 - x) / b


def t_two_sided(t: float, df: float) -> float:
    """P(|T| >= |t|) for Student's t with `df` degrees of freedom: I_{df / (df + t^2)}(df / 2, 1 / 2).  NaN in, NaN out."""
    if not (math.isfinite(t) and df > 0):
        return 0.0 if math.isinf(t) and df > 0 else float("nan")
    return betainc(df / 2.0, 0.5, df / (df + t * t))


def dm_statistic(d: Sequence[float], lags: int) -> Dict[str, float]:
    """The Diebold-Mariano statistic of one loss differential series d_1 .. d_S, in float64:
      gamma_k = (1/S) sum_{t >= k} (d_t - dbar)(d_{t-k} - dbar),   V = gamma_0 + 2 sum_{k=1..q} (1 - k/(q+1)) gamma_k
      DM = dbar / sqrt(V / S) * sqrt((S + 1 - 2h + h(h-1)/S) / S),  h = q + 1,   p two-sided from t with S - 1 d.o.f.
    q is `lags` capped at S - 1.  V <= 0 (a constant series included), S < 2 or a non-finite value give NaN."""
    x = np.asarray(d, dtype=np.float64).reshape(-1)
    S = x.size
    q = max(0, min(int(lags), S - 1))
    out = {"stat": float("nan"), "p": float("nan"), "mean": float(x.mean()) if S else float("nan"), "variance": float("nan"),
           "lags": q, "n": S}
    if S < 2 or not np.isfinite(x).all() or x.max() == x.min():
        return out
    dbar = x.mean()
    c = x - dbar
    V = float(c @ c) / S
    for k in range(1, q + 1):
        V += 2.0 * (1.0 - k / (q + 1.0)) * float(c[k:] @ c[:-k]) / S
    out["variance"] = V
    h = q + 1
    factor = (S + 1 - 2 * h + h * (h - 1) / S) / S
    if not V > 0.0 or not factor > 0.0:
        return out
    out["stat"] = float(dbar / math.sqrt(V / S) * math.sqrt(factor))
    out["p"] = t_two_sided(out["stat"], S - 1)
    return out


# ------------------------------------------------------------------------------------------------ the table
class WindowScores:
    """The (M, S, H, 8) float64 table on the device: for forecast `names[m]`, window s (its DATASET index) and horizon h the
    eight sums of `HorizonMetrics` over the nodes.  Zero until `update` writes a window's rows; a window is overwritten,
    never accumulated.  `L_in`, `L_out`, `stride` (of the dataset, when known) feed the default block length and lags."""

    def __init__(self, num_windows: int, num_horizons: int, names: Sequence[str], scaler=None,
                 device: Union[str, torch.device] = "cuda", L_in: Optional[int] = None, L_out: Optional[int] = None,
                 stride: int = 1):
        from src.evaluation.metrics import _scaler_params
        self.S, self.H, self.names = int(num_windows), int(num_horizons), [str(n) for n in names]
        if min(self.S, self.H, len(self.names)) < 1 or len(set(self.names)) != len(self.names):
            raise ValueError("WindowScores needs at least one window, one horizon and distinct forecast names")
        self.scaler = _scaler_params(scaler)
        self.L_in, self.L_out, self.stride = L_in, L_out, int(stride)
        self.table = torch.zeros(len(self.names), self.S, self.H, STATS, device=device, dtype=torch.float64)

    def index(self, name: str) -> int:
        if name not in self.names:
            raise KeyError(f"no forecast {name!r} among {self.names}")
        return self.names.index(name)

    def update(self, name: str, y_pred_scaled: torch.Tensor, y_true_scaled: torch.Tensor, rows) -> None:
        """Write the rows of a batch: `rows` holds the window (dataset index) of every sample -- a sequence of ints or an
        int64 device tensor; an index outside [0, num_windows) writes nothing and raises `TecmError` at the next check."""
        if not torch.is_tensor(rows):
            rows = torch.tensor([int(r) for r in rows], dtype=torch.int64).to(self.table.device, non_blocking=True)
        window_stats(y_pred_scaled, y_true_scaled, self.table[self.index(name)], rows, 0, self.scaler)

    def merge_(self, group=None) -> "WindowScores":
        """One all-reduce SUM over the ranks of `group`: ranks write disjoint windows into zeros, so the sum is the union."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.table, op=dist.ReduceOp.SUM, group=group)
        return self

    def totals(self, groups: Optional[torch.Tensor] = None, num_groups: Optional[int] = None) -> np.ndarray:
        """The table summed over the windows in ascending order (the identity resample of `tecm_block_bootstrap`, one
        running float64 sum): (M, H, 8), or (M, G, H, 8) per group of windows when `num_groups` is given."""
        G = 1 if num_groups is None else int(num_groups)
        starts = torch.zeros(1, 1, dtype=torch.int32, device=self.table.device)
        out = bootstrap_sums(self.table.view(len(self.names), self.S, self.H * STATS), starts, self.S, groups, G)
        if groups is not None:
            check_device_errors(self.table.device)
        out = out[0].view(len(self.names), G, self.H, STATS).cpu().numpy()
        return out[:, 0] if num_groups is None else out

    def save(self, path: str) -> str:
        """One `.npz` of numpy arrays only (loads without pickle)."""
        mean, scale = self.scaler if self.scaler is not None else (0.0, 1.0)
        np.savez(path, table=self.table.cpu().numpy(), names=np.asarray(self.names), mean=np.float64(mean),
                 scale=np.float64(scale), clip=np.asarray(self.scaler is not None),
                 window=np.asarray([-1 if self.L_in is None else self.L_in, -1 if self.L_out is None else self.L_out,
                                    self.stride], dtype=np.int64))
        return path if path.endswith(".npz") else path + ".npz"

    @classmethod
    def load(cls, path: str, device: Union[str, torch.device] = "cuda") -> "WindowScores":
        with np.load(path, allow_pickle=False) as z:
            table, win = z["table"], z["window"]
            ws = cls(table.shape[1], table.shape[2], [str(n) for n in z["names"]],
                     (float(z["mean"]), float(z["scale"])) if bool(z["clip"]) else None, device,
                     None if win[0] < 0 else int(win[0]), None if win[1] < 0 else int(win[1]), int(win[2]))
            ws.table.copy_(torch.from_numpy(table))
        return ws


# ------------------------------------------------------------------------------------------------ the evaluation
@torch.no_grad()
def score_windows(model: torch.nn.Module, dataset, edge_index: torch.Tensor, batch_size: int, scaler=None,
                  baselines: Sequence = ("mean",), edge_weight: Optional[torch.Tensor] = None,
                  order: Optional[Sequence[int]] = None, group=None):
    """`evaluate_split`'s one pass, which also keeps every forecast's statistics per window: returns (results, scores)
    with `results` exactly what `evaluate_split` returns and `scores` a `WindowScores` whose row of a window is its dataset
    index.  `baselines` as in `evaluate_split` (a fitted `SarimaBaseline` included); `order` and `group` too: a rank scores
    its shard and `merge_` makes every rank's table the whole split's."""
    names = [MODEL_NAME] + [baseline_name(k) for k in baselines]
    box: List[WindowScores] = []

    def per_forecast(name, pred, y, chunk):
        if not box:
            box.append(WindowScores(len(dataset), pred.shape[1], names, scaler, pred.device, dataset.L_in, dataset.L_out,
                                    getattr(dataset, "stride", 1)))
        box[0].update(name, pred, y, chunk)

    hms, _ = _score_pass(model, dataset, edge_index, batch_size, scaler, baselines, edge_weight, order, None, None,
                         per_forecast=per_forecast)
    if not hms:
        raise ValueError("score_windows() on an empty dataset")
    results = {name: hm.merge_(group).compute() for name, hm in hms.items()}
    scores = box[0].merge_(group)
    check_device_errors(scores.table.device)
    return results, scores


def block_bootstrap(scores: WindowScores, replicates: int = 1000, block_len: Optional[int] = None, seed: int = 0,
                    groups: Optional[torch.Tensor] = None, num_groups: int = 1) -> torch.Tensor:
    """R paired circular block-bootstrap resamples of the windows of `scores`: (R, M, G, H, 8) float64 on the device, the
    table summed over each replicate's windows, per group of windows (`groups`: one int32 id in [0, num_groups) per
    window, on the device; None: one group).  The block starts come from a seeded CPU generator (`draw_starts`), so a seed
    means the same resample on every machine, and every forecast sees the same blocks.

    The default `block_len` is min(2 * ceil((L_in + L_out) / stride), max(1, S // 8)) -- twice the span over which two
    windows share data, capped so that at least eight blocks are drawn.  That is a rule of thumb, not an estimate of the
    errors' dependence: intervals from too short a block are too narrow, so try a longer one before trusting a narrow
    interval."""
    if block_len is None:
        if scores.L_in is None or scores.L_out is None:
            raise ValueError("block_len=None needs scores that know their windows' L_in and L_out")
        block_len = default_block_len(scores.S, scores.L_in, scores.L_out, scores.stride)
    starts = draw_starts(scores.S, block_len, replicates, seed).to(scores.table.device)
    M = len(scores.names)
    out = bootstrap_sums(scores.table.view(M, scores.S, scores.H * STATS), starts, int(block_len), groups, int(num_groups))
    check_device_errors(scores.table.device)
    return out.view(int(replicates), M, int(num_groups), scores.H, STATS)


def _averages(stats: np.ndarray) -> Dict[str, np.ndarray]:
    """(..., H, 8) statistics -> the four per-horizon metrics of `derive` and their averages over the horizons."""
    from src.evaluation.metrics import derive
    per = derive(stats)
    out = {k: per[k] for k in ("mae", "rmse", "r2_score", "pearson_r")}
    out.update({f"{k}_avg": per[k].mean(axis=-1) for k in ("mae", "rmse", "r2_score", "pearson_r")})
    return out


def _improvement(m: Dict[str, np.ndarray], b: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """`improvement()` on arrays of averages."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"mae": (b["mae_avg"] - m["mae_avg"]) / b["mae_avg"] * 100,
                "rmse": (b["rmse_avg"] - m["rmse_avg"]) / b["rmse_avg"] * 100,
                "r2_score": (m["r2_score_avg"] - b["r2_score_avg"]) / np.abs(b["r2_score_avg"]) * 100,
                "pearson_r": (m["pearson_r_avg"] - b["pearson_r_avg"]) / b["pearson_r_avg"] * 100}


def _band(point: np.ndarray, reps: np.ndarray, level) -> Dict[str, np.ndarray]:
    lo, hi, nan = percentile_interval(reps, level)
    return {"point": np.asarray(point), "lo": lo, "hi": hi, "nan_replicates": nan}


def bootstrap_intervals(boot: torch.Tensor, scores: WindowScores, level: float = 0.9, model: str = MODEL_NAME,
                        baseline: str = "HistoricalAverage", groups: Optional[torch.Tensor] = None) -> Dict[str, object]:
    """Percentile intervals from the replicates of `block_bootstrap` (`groups`: the ids it was given).  Every replicate goes
    through `derive` (MAE, RMSE, R^2, Pearson r per horizon) and the averages over the horizons.  Returns
      "metrics":     {forecast: {key: band}}, key in mae / rmse / r2_score / pearson_r (arrays (G, H)) and *_avg (G)
      "improvement": {mae / rmse / r2_score / pearson_r: band (G)}: `improvement()`'s percentages of `model` over
                     `baseline`, paired: both from the same resampled windows
      "p_better":    {"mae", "rmse"} (G): the share of replicates in which the model's average is below the baseline's
      "replicates":  {"metrics": {forecast: {*_avg: (R, G)}}, "improvement": {key: (R, G)}}
    with band = {"point" (from `scores.totals()`), "lo", "hi", "nan_replicates"}.  The ends are order statistics of the
    replicates without interpolation, rounded outward (`interval_ranks`); replicates whose value is NaN (a group that a
    resample left empty) are counted in "nan_replicates" and not ranked."""
    b = boot.cpu().numpy()                                                  # (R, M, G, H, 8)
    R, M, G = b.shape[:3]
    if M != len(scores.names) or b.shape[3:] != (scores.H, STATS):
        raise ValueError(f"replicates of shape {b.shape} do not belong to these scores")
    point = scores.totals(groups, G)                                        # (M, G, H, 8)
    rep = {n: _averages(b[:, i]) for i, n in enumerate(scores.names)}
    pt = {n: _averages(point[i]) for i, n in enumerate(scores.names)}
    im, ib = scores.names[scores.index(model)], scores.names[scores.index(baseline)]
    imp_rep, imp_pt = _improvement(rep[im], rep[ib]), _improvement(pt[im], pt[ib])
    p_better = {}
    for k in ("mae", "rmse"):
        a_, b_ = rep[im][f"{k}_avg"], rep[ib][f"{k}_avg"]
        ok = ~(np.isnan(a_) | np.isnan(b_))
        with np.errstate(divide="ignore", invalid="ignore"):
            p_better[k] = ((a_ < b_) & ok).sum(axis=0) / ok.sum(axis=0)
    return {
        "level": float(level), "replicates_count": R, "num_groups": G, "names": list(scores.names), "model": im,
        "baseline": ib,
        "metrics": {n: {k: _band(pt[n][k], rep[n][k], level) for k in rep[n]} for n in scores.names},
        "improvement": {k: _band(imp_pt[k], imp_rep[k], level) for k in IMPROVEMENTS},
        "p_better": p_better,
        "replicates": {"metrics": {n: {k: rep[n][k] for k in AVERAGES} for n in scores.names}, "improvement": imp_rep},
    }


def diebold_mariano(scores: WindowScores, a: str, b: str, loss: str = "se", lags: Optional[int] = None,
                    groups: Optional[torch.Tensor] = None, num_groups: int = 1):
    """The Diebold-Mariano test of forecast `a` against forecast `b` on the loss of every window: d_s = loss_a(s) -
    loss_b(s) with the loss of a window and horizon its mean squared ("se") or absolute ("ae") error over the nodes, from
    the table (sum e^2 / n, sum |e| / n).  Per horizon and pooled (d_s averaged over the horizons) `dm_statistic`: Bartlett
    weights, the Harvey-Leybourne-Newbold factor, two-sided p from Student's t with S - 1 degrees of freedom; negative
    statistics favour `a`.  Default lags: `default_lags` = max(ceil(L_out / stride) - 1, floor(4 (S / 100)^(2/9))).
    Returns {"stat", "p", "mean" (H), "stat_pooled", "p_pooled", "mean_pooled", "lags", "n", "loss"}; V <= 0 (`a` against
    itself) or fewer than two windows give NaN, not an exception.  Windows that were never written (count 0) are left out.
    With `groups` ((S) int32, on the device or host) the result is a list with one entry per group: the test on that group's
    windows in time order, as if they were consecutive -- the gaps between them are ignored.  Float64 on the host."""
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {sorted(LOSSES)}, got {loss!r}")
    ia, ib = scores.index(a), scores.index(b)
    tab = scores.table[[ia, ib]].cpu().numpy()                              # (2, S, H, 8)
    ids = None if groups is None else torch.as_tensor(groups).cpu().numpy().reshape(-1)
    if ids is not None and ids.shape[0] != scores.S:
        raise ValueError(f"groups must hold one id per window ({scores.S})")
    written = (tab[:, :, :, 0] > 0).all(axis=(0, 2))
    out = []
    for g in range(int(num_groups) if ids is not None else 1):
        keep = written if ids is None else written & (ids == g)
        t = tab[:, keep]
        n = int(keep.sum())
        d = t[0, :, :, LOSSES[loss]] / t[0, :, :, 0] - t[1, :, :, LOSSES[loss]] / t[1, :, :, 0]     # (n, H)
        if lags is not None:
            q = int(lags)
        elif scores.L_out is not None:
            q = default_lags(max(n, 1), scores.L_out, scores.stride)
        else:
            q = default_lags(max(n, 1), 1, 1)
        per = [dm_statistic(d[:, h], q) for h in range(scores.H)]
        pooled = dm_statistic(d.mean(axis=1) if n else np.zeros(0), q)
        out.append({"stat": np.array([r["stat"] for r in per]), "p": np.array([r["p"] for r in per]),
                    "mean": np.array([r["mean"] for r in per]), "stat_pooled": pooled["stat"], "p_pooled": pooled["p"],
                    "mean_pooled": pooled["mean"], "lags": pooled["lags"], "n": n, "loss": loss})
    return out if ids is not None else out[0]


@torch.no_grad()
def evaluate_significance(model: torch.nn.Module, dataset, edge_index: torch.Tensor, batch_size: int, scaler=None,
                          baselines: Sequence = ("mean",), edge_weight: Optional[torch.Tensor] = None,
                          order: Optional[Sequence[int]] = None, group=None, replicates: int = 1000,
                          block_len: Optional[int] = None, seed: int = 0, level: float = 0.9, lags: Optional[int] = None,
                          groups: Optional[torch.Tensor] = None, num_groups: int = 1):
    """`evaluate_split` with error bars: returns (results, sig), `results` exactly `evaluate_split`'s.  One pass
    (`score_windows`), one `block_bootstrap`, and against every baseline `bootstrap_intervals` and `diebold_mariano` (both
    losses).  sig: {"scores": the `WindowScores`, "block_len", "replicates", "seed", "level", "num_groups",
    "intervals": {baseline: `bootstrap_intervals`' dict}, "dm": {baseline: {"se": ..., "ae": ...}}} with the
    Diebold-Mariano entries lists over the groups.  `groups`: one int32 id in [0, num_groups) per dataset index, on the
    device, as in `evaluate_maps`."""
    if groups is not None and (groups.dtype != torch.int32 or groups.shape != (len(dataset),)):
        raise ValueError(f"groups must be an int32 tensor with one id per dataset index ({len(dataset)})")
    results, scores = score_windows(model, dataset, edge_index, batch_size, scaler, baselines, edge_weight, order, group)
    if block_len is None:
        block_len = default_block_len(scores.S, scores.L_in, scores.L_out, scores.stride)
    boot = block_bootstrap(scores, replicates, block_len, seed, groups, num_groups)
    ids = groups if groups is not None else torch.zeros(scores.S, dtype=torch.int32)
    sig = {"scores": scores, "block_len": int(block_len), "replicates": int(replicates), "seed": int(seed),
           "level": float(level), "num_groups": int(num_groups), "intervals": {}, "dm": {}}
    for name in scores.names[1:]:
        sig["intervals"][name] = bootstrap_intervals(boot, scores, level, MODEL_NAME, name, groups)
        sig["dm"][name] = {loss: diebold_mariano(scores, MODEL_NAME, name, loss, lags, ids, num_groups) for loss in LOSSES}
    return results, sig


CSV_COLUMNS = ("forecast", "versus", "group", "metric", "point", "lo", "hi", "nan_replicates", "improvement",
               "improvement_lo", "improvement_hi", "p_better", "dm_stat", "dm_p", "dm_lags")
_DM_LOSS = {"mae": "ae", "rmse": "se"}


def write_significance(sig: Dict[str, object], output_dir: str) -> Dict[str, str]:
    """The files of `evaluate_significance`'s second result.  `significance.csv`: one line per forecast, group and metric
    (the four averages) with point, lo, hi; for the model one such line per baseline it is compared with ("versus"), with
    the improvement and its interval and, for MAE and RMSE, `p_better` and the pooled Diebold-Mariano statistic, p-value and
    lags of the matching loss (absolute / squared error).  `significance.npz`: the replicates' arrays
    `<forecast>/<metric>_avg` and `improvement/<baseline>/<key>`, each (R, G).  numpy and the standard library only."""
    os.makedirs(output_dir, exist_ok=True)
    csv_path = os.path.join(output_dir, "significance.csv")
    arrays = {}
    f64 = lambda v: repr(float(v))                                          # noqa: E731
    with open(csv_path, "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow(CSV_COLUMNS)
        done = set()
        for base, iv in sig["intervals"].items():
            for name in iv["names"]:
                is_model = name == iv["model"]
                if not is_model and name in done:
                    continue
                done.add(name)
                for g in range(iv["num_groups"]):
                    for key in AVERAGES:
                        band, short = iv["metrics"][name][key], key[:-4]
                        row = [name, base if is_model else "", g, key, f64(band["point"][g]), f64(band["lo"][g]),
                               f64(band["hi"][g]), int(band["nan_replicates"][g])]
                        if is_model:
                            imp = iv["improvement"][short]
                            row += [f64(imp["point"][g]), f64(imp["lo"][g]), f64(imp["hi"][g])]
                            if short in _DM_LOSS:
                                dm = sig["dm"][base][_DM_LOSS[short]][g]
                                row += [f64(iv["p_better"][short][g]), f64(dm["stat_pooled"]), f64(dm["p_pooled"]), dm["lags"]]
                        wr.writerow(row + [""] * (len(CSV_COLUMNS) - len(row)))
                for key in AVERAGES:
                    arrays[f"{name}/{key}"] = iv["replicates"]["metrics"][name][key]
            for key in IMPROVEMENTS:
                arrays[f"improvement/{base}/{key}"] = iv["replicates"]["improvement"][key]
    npz_path = os.path.join(output_dir, "significance.npz")
    np.savez_compressed(npz_path, **arrays)
    return {"csv": csv_path, "npz": npz_path}
