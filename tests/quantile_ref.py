"""A float64 numpy restatement of the quantile kernels (include/tecmollm.h (3k)), written from the formulas there and adding
in the kernels' order: the pinball loss pair, `tecm_quantile_stats` and the CQR score.  No code shared with csrc/."""
from __future__ import annotations

import numpy as np

BLOCK_CAP = 1024                     # TECM_PINBALL_BLOCK_CAP
TEC_MIN, TEC_MAX = np.float32(0.0), np.float32(200.0)


# ------------------------------------------------------------------------------------------------ pinball
def _butterfly(v):
    """64 doubles -> their sum in the order of six halvings v[l] += v[l ^ o], o = 32 .. 1."""
    v = np.array(v, dtype=np.float64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[np.arange(64) ^ o]
    return v[0]


def _block_sum(t256):
    w = [_butterfly(t256[64 * k:64 * k + 64]) for k in range(4)]
    return (w[0] + w[1]) + (w[2] + w[3])


def pinball(pred, target, taus, grad_scale=1.0, h_fast=True):
    """pred (B, Q, H, N), target (B, H, N) float32 -> (loss f32, loss_levels (Q) f32, dpred (B, Q, H, N) f32, mags): the mean
    pinball loss in the kernel's order of additions (`h_fast`: the order in which a level's elements are walked, h fastest
    for the head's storage, n fastest when the nodes are contiguous); mags = (sum |rho| per level) for the tolerance."""
    pred, target = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    B, Q, H, N = pred.shape
    M = B * H * N
    tau32 = np.asarray(taus, np.float32)
    u = target[:, None] - pred                                             # float32
    neg = u < 0
    rho = u.astype(np.float64) * (tau32.astype(np.float64)[None, :, None, None] - neg)
    g = np.float32(grad_scale) / np.float32(M * Q)
    dpred = (g * (neg.astype(np.float32) - tau32[None, :, None, None])).astype(np.float32)
    nbx = min((M + 255) // 256, BLOCK_CAP)
    levels, total, mags = np.zeros(Q, np.float32), 0.0, np.zeros(Q)
    for q in range(Q):
        r = rho[:, q]                                                      # (B, H, N)
        flat = (r.transpose(0, 2, 1) if h_fast else r).reshape(-1)         # element e of the level's space
        mags[q] = np.abs(flat).sum()
        pad = np.zeros(-(-M // (nbx * 256)) * nbx * 256)
        pad[:M] = flat
        per_thread = np.zeros(nbx * 256)
        for row in pad.reshape(-1, nbx * 256):                             # ascending e per thread
            per_thread = per_thread + row
        partial = np.array([_block_sum(per_thread[256 * x:256 * x + 256]) for x in range(nbx)])
        t2 = np.zeros(256)
        for x0 in range(0, nbx, 256):
            chunk = partial[x0:x0 + 256]
            t2[:chunk.size] = t2[:chunk.size] + chunk
        level = _block_sum(t2)
        levels[q] = np.float32(level / M)
        total += level
    return np.float32(total / (Q * float(M))), levels, dpred, mags


# ------------------------------------------------------------------------------------------------ value pipeline
def unscale(v, scaler):
    """Raw scaled float32 -> physical float32: two float32 roundings, then nan_to_num (NaN -> 0, +inf -> 100, -inf -> 0)."""
    v = np.asarray(v, np.float32)
    if scaler is not None:
        mean, scale = scaler
        a = (v.astype(np.float64) * scale).astype(np.float32)
        v = (a.astype(np.float64) + mean).astype(np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    v = np.where(np.isposinf(v), np.float32(100), v)
    return np.where(np.isneginf(v), np.float32(0), v).astype(np.float32)


def values(levels, target, scaler):
    """levels (S, Q, H, I), target (S, H, I) raw -> x (S, Q, H, I), y (S, H, I) float32 in physical units: non-finite level
    -> 0 first, the inverse transform, nan_to_num, and the clip of the levels only (with a scaler)."""
    lv = np.asarray(levels, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        x = unscale(np.where(np.isfinite(lv), lv, np.float32(0)), scaler)
        y = unscale(target, scaler)
    if scaler is not None:
        x = np.minimum(np.maximum(x, TEC_MIN), TEC_MAX)
    return x, y


def sorted_levels(levels, target, scaler, adjust=None, ids=None):
    """-> z (S, Q, H, I) sorted ascending (+ adjust[(g or 0), h, q, i] in float32), y (S, H, I), crossing (S, H, I) bool."""
    x, y = values(levels, target, scaler)
    crossing = (x[:, :-1] > x[:, 1:]).any(axis=1) if x.shape[1] > 1 else np.zeros(y.shape, bool)
    z = np.sort(x, axis=1)
    if adjust is not None:
        adj = np.asarray(adjust, np.float32)                               # (Ga, H, Q, I)
        S = z.shape[0]
        g = np.zeros(S, np.int64) if (ids is None or adj.shape[0] == 1) else np.clip(np.asarray(ids, np.int64), 0, adj.shape[0] - 1)
        with np.errstate(invalid="ignore"):
            z = (z + adj[g].transpose(0, 2, 1, 3)).astype(np.float32)
    return z, y, crossing


def accumulate(stats, counts, mags, levels, target, taus, ids, scaler, adjust=None):
    """One `tecm_quantile_stats` call on numpy stats / mags (G, H, 1 + Q + P, I) float64 and counts (same shape) int64: the
    samples of a cell are added in ascending s.  mags collects sum |term| for the tolerance.  Returns z."""
    G = stats.shape[0]
    z, y, crossing = sorted_levels(levels, target, scaler, adjust, ids)
    S, Q = z.shape[:2]
    P = Q // 2
    tau = np.asarray(taus, np.float32).astype(np.float64)
    yd, zd = y.astype(np.float64), z.astype(np.float64)
    for s in range(S):
        g = 0 if ids is None else int(ids[s])
        if not 0 <= g < G:
            continue
        stats[g, :, 0] += 1.0
        mags[g, :, 0] += 1.0
        counts[g, :, 0] += crossing[s]
        for q in range(Q):
            with np.errstate(invalid="ignore"):
                rho = (yd[s] - zd[s, q]) * (tau[q] - (y[s] < z[s, q]))
            stats[g, :, 1 + q] += rho
            mags[g, :, 1 + q] += np.abs(rho)
            counts[g, :, 1 + q] += y[s] <= z[s, q]
        for r in range(P):
            lo, hi = z[s, r], z[s, Q - 1 - r]
            with np.errstate(invalid="ignore"):
                w = hi.astype(np.float64) - lo.astype(np.float64)
            stats[g, :, 1 + Q + r] += w
            mags[g, :, 1 + Q + r] += np.abs(w)
            counts[g, :, 1 + Q + r] += (lo <= y[s]) & (y[s] <= hi)
    return z


def cqr_scores(levels, target, lo_idx, hi_idx, scaler):
    """E = max(z_lo - y, y - z_hi) in float32, (S, H, I)."""
    z, y, _ = sorted_levels(levels, target, scaler)
    return np.maximum(z[:, lo_idx] - y, y - z[:, hi_idx]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ derived scores
def winkler_direct(lo, hi, y, alpha):
    """width + (2 / alpha) (lo - y)_+ + (2 / alpha) (y - hi)_+, float64."""
    lo, hi, y = (np.asarray(a, np.float64) for a in (lo, hi, y))
    return (hi - lo) + (2 / alpha) * np.maximum(lo - y, 0) + (2 / alpha) * np.maximum(y - hi, 0)


def rho(y, z, tau):
    y, z = np.asarray(y, np.float64), np.asarray(z, np.float64)
    return (y - z) * (tau - (y < z))
