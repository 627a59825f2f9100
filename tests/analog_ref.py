"""float64 numpy restatement of the analog ensemble `AnalogBaseline` searches and forecasts on the device
(include/tecmollm.h (10)): the sliding-window squared distances, the admission rules (keys, exclusion, finiteness), the
selection of the K smallest by (distance, row) with `np.lexsort`, the members and their mean.  Written from the formulas,
not from the kernels; series are time-major (T, N) here."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

MAX_K, MAX_M, MAX_H = 32, 512, 32


def n_candidates(Ta, Ty, m, L_out):
    """Start rows c with 0 <= c, c + m <= Ta and c + m + L_out <= Ty."""
    return max(min(Ta, Ty - L_out) - m + 1, 0)


def segments(Xq, starts, L_in, m):
    """Xq (Tq, N) -> (S, m, N): the last m input steps of the windows that start at `starts`."""
    starts = np.asarray(starts, dtype=np.int64)
    return np.stack([np.asarray(Xq)[a + L_in - m:a + L_in] for a in starts])


def distances(A, seg, ncand):
    """A (Ta, N), seg (m, N) -> (ncand, N) float64: d[c, n] = sum_l (A[c + l, n] - seg[l, n])^2."""
    A, seg = np.asarray(A, dtype=np.float64), np.asarray(seg, dtype=np.float64)
    m, N = seg.shape
    out = np.empty((ncand, N))
    if ncand == 0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(N):
            w = sliding_window_view(A[:ncand + m - 1, n], m)               # (ncand, m)
            out[:, n] = ((w - seg[None, :, n]) ** 2).sum(axis=1)
    return out


def admitted(ncand, m, key_arch=None, key_q=None, exclude=0, o_q=None):
    """(ncand,) bool: key_arch[o_c] == key_q and |o_c - o_q| >= exclude, with o_c = c + m."""
    o_c = np.arange(ncand, dtype=np.int64) + m
    ok = np.ones(ncand, dtype=bool)
    if key_arch is not None:
        ok &= np.asarray(key_arch)[o_c] == key_q
    if exclude > 0:
        ok &= np.abs(o_c - int(o_q)) >= exclude
    return ok


def search(A, Ty, segs, K, L_out, key_arch=None, key_q=None, exclude=0, o_q=None, want_all=False):
    """A (Ta, N), segs (S, m, N) -> idx (S, N, K) int32, dist (S, N, K) float64, count (S, N) int32: per (query, node) the K
    admitted candidates with a finite distance smallest by (d, c), ascending; unused places -1 / +inf.  With `want_all`
    also the masked distance table (S, ncand, N) (+inf where not admitted or not finite)."""
    A = np.asarray(A)
    S, m, N = segs.shape
    ncand = n_candidates(A.shape[0], Ty, m, L_out)
    idx = np.full((S, N, K), -1, dtype=np.int32)
    dist = np.full((S, N, K), np.inf)
    count = np.zeros((S, N), dtype=np.int32)
    table = np.full((S, ncand, N), np.inf) if want_all else None
    c = np.arange(ncand)
    for s in range(S):
        d = distances(A, segs[s], ncand)
        ok = admitted(ncand, m, key_arch, None if key_q is None else key_q[s], exclude, None if o_q is None else o_q[s])
        d = np.where(ok[:, None] & np.isfinite(d), d, np.inf)
        if want_all:
            table[s] = d
        for n in range(N):
            order = np.lexsort((c, d[:, n]))[:K]                           # by d, then by c
            order = order[np.isfinite(d[order, n])]
            idx[s, n, :len(order)], dist[s, n, :len(order)], count[s, n] = order, d[order, n], len(order)
    return (idx, dist, count, table) if want_all else (idx, dist, count)


def forecast(Y, idx, count, m, L_out):
    """Y (Ty, N) -> members (K, S, L_out, N) float64 (NaN beyond count), mean (S, L_out, N) (NaN where count == 0)."""
    Y = np.asarray(Y, dtype=np.float64)
    S, N, K = idx.shape
    members = np.full((K, S, L_out, N), np.nan)
    n_ix = np.arange(N)
    for k in range(K):
        for h in range(L_out):
            live = k < count                                                # (S, N)
            rows = np.where(live, idx[:, :, k].astype(np.int64) + m + h, 0)
            members[k, :, h, :] = np.where(live, Y[rows, n_ix[None, :]], np.nan)
    mean = np.full((S, L_out, N), np.nan)
    for s in range(S):
        for n in range(N):
            if count[s, n] > 0:
                mean[s, :, n] = members[:count[s, n], s, :, n].mean(axis=0)
    return members, mean


def integer_series(T, N, seed, bound=8):
    """(T, N) float32 of integers in [-bound, bound]: every difference, square and sum of up to 512 squares is exact in fp32."""
    return np.random.default_rng(seed).integers(-bound, bound + 1, (T, N)).astype(np.float32)


def rmse(pred, truth):
    return float(np.sqrt(np.nanmean((np.asarray(pred, dtype=np.float64) - np.asarray(truth, dtype=np.float64)) ** 2)))


def held_out_scores(y, slots, L_in=48, H=12, K=16, m=48):
    """The sanity recipe on a (T, N) series that is both the input channel and the target: the archive is the record behind
    the first two thirds of the stride-1 windows, the last third is scored with slot keys `slots` (T,).
    {"analog", "mean"}: RMSE over every window, horizon and node."""
    T = y.shape[0]
    S = T - L_in - H + 1
    n_fit = 2 * S // 3
    Ta, Ty = (n_fit - 1) + L_in, (n_fit - 1) + L_in + H
    test = np.arange(n_fit, S)
    segs = segments(y, test, L_in, m)
    key_arch = slots[:Ta + 1].astype(np.int32)
    idx, _, count = search(y[:Ta], Ty, segs, K, H, key_arch, slots[test + L_in].astype(np.int32))
    _, mean = forecast(y[:Ty], idx, count, m, H)
    truth = np.stack([y[a + L_in:a + L_in + H] for a in test])              # (B, H, N)
    window_mean = np.stack([np.repeat(y[a:a + L_in].astype(np.float64).mean(axis=0)[None], H, axis=0) for a in test])
    return {"analog": rmse(mean, truth), "mean": rmse(window_mean, truth), "min_count": int(count.min())}
