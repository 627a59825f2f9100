"""numpy restatement of the per-cell evaluation statistics (tecm_metrics_map), shared by tests/test_host_error_maps.py and
tests/test_gpu_error_maps.py: the value pipeline in float32 as the kernel runs it, the eight sums in float64 added in the
kernel's order (ascending update, then ascending sample)."""
import numpy as np

F32, F64 = np.float32, np.float64


def _unscale(y, mean, scale):
    a = (y.astype(F64) * scale).astype(F32)                               # X *= scale_ ; X += mean_: two f32 roundings
    return (a.astype(F64) + mean).astype(F32)


def pipeline(pred, true, scaler=None):
    """Scaled float32 (S, H, I) arrays -> (t, p) float32 in physical units, as metrics.py:137-143, :36-51 leave them."""
    mean, scale = scaler if scaler is not None else (0.0, 1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.where(np.isfinite(pred), pred, F32(0)).astype(F32)
        p = np.nan_to_num(_unscale(p, mean, scale), nan=0.0, posinf=100.0, neginf=0.0)
        t = np.nan_to_num(_unscale(np.asarray(true, dtype=F32), mean, scale), nan=0.0, posinf=100.0, neginf=0.0)
    if scaler is not None:
        p = np.clip(p, F32(0), F32(200))
    return t.astype(F32), p.astype(F32)


def terms(t, p):
    """(8, ...) float64: what one (t, p) pair adds to [n, St, Sp, Stt, Spp, Stp, S|t-p|, S(t-p)^2]."""
    t, p = t.astype(F64), p.astype(F64)
    d = t - p
    return np.stack([np.ones_like(t), t, p, t * t, p * p, t * p, np.abs(d), d * d])


def accumulate(stats, mags, pred, true, groups=None, scaler=None):
    """One update into stats / mags, both (G, H, 8, I) float64: stats as the kernel adds them, mags the sum of the
    terms' absolute values (the scale of the rounding-error bar).  A sample whose id is outside [0, G) is skipped."""
    t, p = pipeline(pred, true, scaler)
    G = stats.shape[0]
    for s in range(t.shape[0]):
        g = 0 if groups is None else int(groups[s])
        if not 0 <= g < G:
            continue
        k = terms(t[s], p[s])                                             # (8, H, I)
        stats[g] += k.transpose(1, 0, 2)
        mags[g] += np.abs(k).transpose(1, 0, 2)
