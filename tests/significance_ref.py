"""numpy float64 restatement of the significance feature (tecm_metrics_window, tecm_block_bootstrap and the host arithmetic
of tecmollm/significance.py), shared by tests/test_host_significance.py and tests/test_gpu_significance.py: the value
pipeline of tests/error_maps_ref.py, the per-window sums in the kernel's documented order (a lane's nodes in ascending
order, then the butterfly over the 64 lanes), the bootstrap's row sequence and its sequential sums, `derive`-based metrics,
order-statistic intervals, the Diebold-Mariano statistic and Student's t tail (by the finite series of Abramowitz & Stegun
26.7.3 / 26.7.4 for an integer number of degrees of freedom -- not the incomplete beta function the package uses)."""
import math

import numpy as np

from tests.error_maps_ref import pipeline, terms

F64 = np.float64
LANES = 64


def window_table(pred, true, scaler=None):
    """Scaled float32 (S, H, I) arrays -> (table, mags), both (S, H, 8) float64: the eight sums of every (sample, horizon)
    over the nodes as the kernel adds them, and the sums of the terms' absolute values (the scale of the error bar)."""
    t, p = pipeline(pred, true, scaler)
    k = terms(t, p)                                                        # (8, S, H, I)
    S, H, I = t.shape
    tiles = -(-I // LANES)
    padded = np.zeros((8, S, H, tiles * LANES), dtype=F64)                 # a lane without a node adds nothing: x + 0.0 = x,
    padded[..., :I] = k                                                    # and a partial that starts at +0.0 is never -0.0
    padded = padded.reshape(8, S, H, tiles, LANES)
    part = np.zeros((8, S, H, LANES), dtype=F64)
    for j in range(tiles):                                                 # lane l: nodes l, l + 64, ... in ascending order
        part = part + padded[:, :, :, j]
    width = LANES
    while width > 1:                                                       # x[l] += x[l ^ o], o = 32 .. 1: halves
        width //= 2
        part = part[..., :width] + part[..., width:2 * width]
    table = part[..., 0].transpose(1, 2, 0)
    mags = np.abs(k).sum(axis=3).transpose(1, 2, 0)
    return np.ascontiguousarray(table), np.ascontiguousarray(mags)


def bootstrap_rows(starts, S, L):
    """Position t = k*L + j reads window (starts[k] + j) mod S, t = 0 .. S-1; None for a start outside [0, S)."""
    assert len(starts) == -(-S // L)
    rows = []
    for t in range(S):
        st = int(starts[t // L])
        rows.append((st + t % L) % S if 0 <= st < S else None)
    return rows


def bootstrap_sums(table, starts, L, groups=None, G=1):
    """(M, S, W) float64, starts (R, K) -> (R, M, G, W): one running sum per output value, added in ascending t.  A bad
    start or a group id outside [0, G) skips the window."""
    M, S, W = table.shape
    out = np.zeros((len(starts), M, G, W), dtype=F64)
    for r, st in enumerate(starts):
        for row in bootstrap_rows(st, S, L):
            if row is None:
                continue
            g = 0 if groups is None else int(groups[row])
            if 0 <= g < G:
                out[r, :, g, :] += table[:, row, :]
    return out


def interval_ranks(R, level=0.9):
    """0-based ranks floor((alpha/2)(R-1)) and ceil((1-alpha/2)(R-1)) in integer arithmetic; level given in per mille."""
    half = round((1 - level) * 1000)                                       # alpha in per mille; alpha / 2 = half / 2000
    lo = (half * (R - 1)) // 2000
    hi = -((-(2000 - half) * (R - 1)) // 2000)
    return lo, hi


def interval(values, level=0.9):
    """Order statistics of the non-NaN values of a 1-D array: (lo, hi, number of NaNs)."""
    v = np.asarray(values, dtype=F64)
    ok = np.sort(v[~np.isnan(v)])
    if ok.size == 0:
        return np.nan, np.nan, v.size
    lo, hi = interval_ranks(ok.size, level)
    return ok[lo], ok[hi], v.size - ok.size


def averages(stats):
    """(..., H, 8) -> {"mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg"} over the leading axes, through `derive`."""
    from src.evaluation.metrics import derive
    per = derive(stats)
    return {f"{k}_avg": per[k].mean(axis=-1) for k in ("mae", "rmse", "r2_score", "pearson_r")}


def t_two_sided(t, df):
    """P(|T| >= |t|), integer df >= 1: 1 - A(t | df) with A from Abramowitz & Stegun 26.7.3 (odd df) / 26.7.4 (even df)."""
    df = int(df)
    theta = math.atan(abs(t) / math.sqrt(df))
    s, c2 = math.sin(theta), math.cos(theta) ** 2
    if df % 2 == 0:
        term, total = 1.0, 1.0
        for j in range(1, df // 2):                                        # 1 + 1/2 c^2 + (1*3)/(2*4) c^4 + ... to c^(df-2)
            term *= (2 * j - 1) / (2 * j) * c2
            total += term
        return 1.0 - s * total
    if df == 1:
        return 1.0 - 2.0 * theta / math.pi
    term, total = 1.0, 1.0
    for j in range(1, (df - 1) // 2):                                      # 1 + 2/3 c^2 + (2*4)/(3*5) c^4 + ... to c^(df-3)
        term *= (2 * j) / (2 * j + 1) * c2
        total += term
    return 1.0 - 2.0 / math.pi * (theta + s * math.cos(theta) * total)


def dm(d, q):
    """(statistic, two-sided p) of the loss differential series d with q Bartlett lags and the HLN factor; NaN when V <= 0."""
    d = [float(v) for v in d]
    S = len(d)
    if S < 2:
        return math.nan, math.nan
    q = min(q, S - 1)
    dbar = math.fsum(d) / S
    c = [v - dbar for v in d]
    gamma = [math.fsum(c[t] * c[t - k] for t in range(k, S)) / S for k in range(q + 1)]
    V = gamma[0] + 2.0 * sum((1.0 - k / (q + 1.0)) * gamma[k] for k in range(1, q + 1))
    h = q + 1
    factor = (S + 1 - 2 * h + h * (h - 1) / S) / S
    if max(d) == min(d) or not V > 0 or not factor > 0:
        return math.nan, math.nan
    stat = dbar / math.sqrt(V / S) * math.sqrt(factor)
    return stat, t_two_sided(stat, S - 1)


def ar1_columns(S=512, C=400, phi=0.6, seed=20261020):
    """(S, C) float64: C independent stationary AR(1) series with unit innovations, mean 0."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((S, C))
    x = np.empty((S, C), dtype=F64)
    x[0] = e[0] / math.sqrt(1.0 - phi * phi)
    for t in range(1, S):
        x[t] = phi * x[t - 1] + e[t]
    return x


def coverage_of_zero(sums, S, level=0.9):
    """(R, C) resampled sums of mean-0 columns -> the share of columns whose percentile interval of the mean covers 0."""
    means = np.sort(np.asarray(sums, dtype=F64) / S, axis=0)
    lo, hi = interval_ranks(means.shape[0], level)
    return float(((means[lo] <= 0) & (0 <= means[hi])).mean())
