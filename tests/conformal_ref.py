"""numpy restatement of the conformal kernels (include/tecmollm.h (3g)), shared by tests/test_host_conformal.py and
tests/test_gpu_conformal.py: the value pipeline in its float32 roundings (tests/error_maps_ref.py), the scores in float32,
the selection per group by `np.sort` (numeric order, -0 and +0 equal, every NaN last), and the six interval statistics in
float64 added in the kernel's order (ascending update, then ascending sample)."""
import numpy as np

from tests.error_maps_ref import pipeline

F32, F64 = np.float32, np.float64
STATS = 6
MODES = ("absolute", "signed")


def weight(sigma, sigma_min, shape):
    """w = max(sigma, sigma_min) in float32 (a NaN sigma counts as sigma_min); ones without sigma."""
    if sigma is None:
        return np.ones(shape, dtype=F32)
    return np.fmax(np.asarray(sigma, dtype=F32), F32(sigma_min)).astype(F32)


def scores(pred, true, scaler=None, mode="absolute", sigma=None, sigma_min=1e-3):
    """Scaled float32 (S, H, I) arrays -> (r, p, y, w), all float32: one f32 subtraction, |.| in the absolute mode, one f32
    division with a sigma."""
    y, p = pipeline(pred, true, scaler)
    w = weight(sigma, sigma_min, p.shape)
    with np.errstate(all="ignore"):
        r = (y - p).astype(F32)
        if mode == "absolute":
            r = np.abs(r)
        if sigma is not None:
            r = (r / w).astype(F32)
    return r, p, y, w


def select(x, ranks, groups=None, G=1):
    """x (S, C) float32, ranks (G, Q) 1-based, groups (S) or None -> (Q, G, C) float32: -inf for a rank <= 0, +inf for a rank
    above the group's row count, the sorted column's entry otherwise.  A row whose id is outside [0, G) is in no group."""
    x = np.asarray(x, dtype=F32)
    ranks = np.asarray(ranks).reshape(G, -1)
    ids = np.zeros(x.shape[0], dtype=np.int64) if groups is None else np.asarray(groups)
    out = np.empty((ranks.shape[1], G, x.shape[1]), dtype=F32)
    for g in range(G):
        srt = np.sort(x[ids == g], axis=0)
        n = srt.shape[0]
        for q, k in enumerate(ranks[g]):
            out[q, g] = -np.inf if k <= 0 else (np.inf if k > n else srt[int(k) - 1])
    return out


def interval_terms(p, y, w, r, q_lo, q_hi, mode, alpha, clip):
    """Per (sample, cell): (6, ...) float64 terms [1, covered, below, above, width, Winkler] and the float32 lo, hi."""
    with np.errstate(all="ignore"):
        lo = (p.astype(F64) + q_lo.astype(F64) * w.astype(F64)).astype(F32)
        hi = (p.astype(F64) + q_hi.astype(F64) * w.astype(F64)).astype(F32)
        if clip:
            lo, hi = np.clip(lo, F32(0), F32(200)), np.clip(hi, F32(0), F32(200))
        if mode == "absolute":
            cov = r <= q_hi
            below = ~cov & (y < p)
        else:
            cov = (q_lo <= r) & (r <= q_hi)
            below = ~cov & (r < q_lo)
        above = ~cov & ~below
        width = hi.astype(F64) - lo.astype(F64)
        yd, pen = y.astype(F64), 2.0 / alpha
        wink = width + pen * np.maximum(lo.astype(F64) - yd, 0.0) + pen * np.maximum(yd - hi.astype(F64), 0.0)
    one = np.ones_like(width)
    return np.stack([one, cov.astype(F64), below.astype(F64), above.astype(F64), width, wink]), lo, hi


def accumulate(stats, mags, pred, true, q_lo, q_hi, alpha, mode="absolute", groups=None, scaler=None, sigma=None,
               sigma_min=1e-3):
    """One update into stats / mags, both (G, H, 6, I) float64, as the kernel adds them; q_lo / q_hi (Gq, H, I) float32 with
    Gq = 1 or G (q_lo None in the absolute mode: -q_hi).  A sample whose id is outside [0, G) is skipped.  Returns the
    per-sample (lo, hi, p), float32 (S, H, I)."""
    r, p, y, w = scores(pred, true, scaler, mode, sigma, sigma_min)
    q_hi = np.asarray(q_hi, dtype=F32)
    q_lo = -q_hi if q_lo is None else np.asarray(q_lo, dtype=F32)
    G = stats.shape[0]
    lo_all, hi_all = np.zeros_like(p), np.zeros_like(p)
    for s in range(p.shape[0]):
        g = 0 if groups is None else int(groups[s])
        if not 0 <= g < G:
            continue
        gq = g if q_hi.shape[0] == G else 0
        k, lo_all[s], hi_all[s] = interval_terms(p[s], y[s], w[s], r[s], q_lo[gq], q_hi[gq], mode, alpha, scaler is not None)
        with np.errstate(all="ignore"):
            stats[g] += k.transpose(1, 0, 2)
            mags[g] += np.abs(k).transpose(1, 0, 2)
    return lo_all, hi_all, p
