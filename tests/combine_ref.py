"""A float64 numpy restatement of the forecast-combination kernels (include/tecmollm.h (3l)), written from the formulas:
the moments added in the kernel's order (ascending sample), the solve with its drop rule (a Cholesky factorisation in member
order, not `lstsq`), and the blend.  Shared by tests/test_host_combine.py and tests/test_gpu_combine.py."""
import numpy as np

from tests import linear_ref as LR

MAX_MEMBERS = 8
EMPTY, FEW, DROPPED, NONFINITE = 1, 2, 4, 8
PIVOT_TOL = 1e-10


def moment_count(M):
    return (M + 2) * (M + 3) // 2 + 1


def moment_index(M, a, b):
    """Moment (a, b), a <= b, of z = [1, p_1 .. p_M, t]: row-major upper triangle."""
    return a * (M + 2) - a * (a - 1) // 2 + (b - a)


def moments(preds, y, groups=None, G=1, stats=None, absolute=False):
    """preds: M arrays (S, H, I) float32, y likewise -> stats (G, H, K, I) float64 (added to `stats` when given).  Per cell
    one running sum per moment, samples in ascending s, float32 x float32 products exact in float64; a sample with a
    non-finite member or target is left out and counted in the last entry; an id outside [0, G) is skipped.
    absolute=True sums |terms| instead (the scale of the error bar)."""
    M = len(preds)
    S, H, I = y.shape
    K = moment_count(M)
    acc = np.zeros((G, H, K, I))
    z = np.ones((M + 2, S, H, I))
    for m, p in enumerate(preds):
        z[1 + m] = np.broadcast_to(p, (S, H, I)).astype(np.float64)
    z[M + 1] = y.astype(np.float64)
    finite = np.isfinite(z).all(axis=0)                                    # (S, H, I)
    ids = np.zeros(S, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            g = ids[s]
            if not 0 <= g < G:
                continue
            ok = finite[s]
            for a in range(M + 2):
                for b in range(a, M + 2):
                    term = z[a, s] * z[b, s]
                    if absolute:
                        term = np.abs(term)
                    acc[g, :, moment_index(M, a, b), :] += np.where(ok, term, 0.0)
            acc[g, :, K - 1, :] += np.where(ok, 0.0, 1.0)
    if stats is None:
        return acc
    present = np.zeros(G, dtype=bool)
    present[ids[(ids >= 0) & (ids < G)]] = True
    out = stats.copy()
    out[present] += acc[present]                                           # a group that does not occur is not touched
    return out


def system(stats, ridge, w0):
    """stats (..., K) -> n, pbar (..., M), tbar, A (..., M, M), b (..., M) by the formulas, in the kernel's operation order."""
    K = stats.shape[-1]
    M = next(m for m in range(1, MAX_MEMBERS + 1) if moment_count(m) == K)
    at = lambda a, b: stats[..., moment_index(M, a, b)]
    n = at(0, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        pbar = np.stack([at(0, 1 + m) / n for m in range(M)], axis=-1)
        tbar = at(0, M + 1) / n
        rn = ridge * n
        A = np.zeros(stats.shape[:-1] + (M, M))
        b = np.zeros(stats.shape[:-1] + (M,))
        for m in range(M):
            b[..., m] = (at(1 + m, M + 1) - n * pbar[..., m] * tbar) + rn * w0[m]
            for k in range(m + 1):
                c = at(1 + k, 1 + m) - n * pbar[..., k] * pbar[..., m]
                if k == m:
                    c = c + rn
                A[..., m, k] = A[..., k, m] = c
    return M, n, pbar, tbar, A, b


def solve(stats, ridge=0.0, w0=None):
    """stats (G, H, K, I) -> weight (G, H, M, I), intercept, status, dropped (G, H, I), cond (G, H, I; the 2-norm condition
    number of the kept system, NaN on a fallback).  Member m is dropped when A_mm <= 0 or its pivot A_mm - sum over kept
    k < m of L_mk^2 is <= 1e-10 A_mm."""
    st = np.moveaxis(np.asarray(stats, dtype=np.float64), 2, -1)           # (G, H, I, K)
    K = st.shape[-1]
    M = next(m for m in range(1, MAX_MEMBERS + 1) if moment_count(m) == K)
    w0 = np.full(M, 1.0 / M) if w0 is None else np.asarray(w0, dtype=np.float64)
    shape = st.shape[:-1]
    weight = np.zeros(shape + (M,))
    intercept = np.zeros(shape)
    status = np.zeros(shape, dtype=np.int32)
    dropped = np.zeros(shape, dtype=np.uint8)
    cond = np.full(shape, np.nan)
    _, n_all, pbar_all, tbar_all, A_all, b_all = system(st, ridge, w0)
    for cell in np.ndindex(*shape):
        s = st[cell]
        if not np.isfinite(s[:K - 1]).all():
            status[cell], weight[cell] = NONFINITE, w0
            continue
        n = n_all[cell]
        if n == 0:
            status[cell], weight[cell] = EMPTY, w0
            continue
        pbar, tbar = pbar_all[cell], tbar_all[cell]
        if n < M + 2:
            status[cell], weight[cell] = FEW, w0
        else:
            A, b = A_all[cell], b_all[cell]
            L = np.zeros((M, M))
            kept = []
            for m in range(M):
                piv = A[m, m]
                for k in kept:
                    piv = piv - L[m, k] * L[m, k]
                if A[m, m] <= 0 or piv <= PIVOT_TOL * A[m, m]:
                    dropped[cell] |= 1 << m
                    continue
                L[m, m] = np.sqrt(piv)
                for j in range(m + 1, M):
                    v = A[j, m]
                    for k in kept:
                        v = v - L[j, k] * L[m, k]
                    L[j, m] = v / L[m, m]
                kept.append(m)
            yv = np.zeros(M)
            for m in kept:
                v = b[m]
                for k in kept:
                    if k < m:
                        v = v - L[m, k] * yv[k]
                yv[m] = v / L[m, m]
            w = np.zeros(M)
            for m in reversed(kept):
                v = yv[m]
                for j in kept:
                    if j > m:
                        v = v - L[j, m] * w[j]
                w[m] = v / L[m, m]
            weight[cell] = w
            if dropped[cell]:
                status[cell] = DROPPED
            if kept:
                cond[cell] = np.linalg.cond(A[np.ix_(kept, kept)])
        dot = 0.0
        for m in range(M):
            dot = dot + weight[cell][m] * pbar[m]
        intercept[cell] = tbar - dot
    return np.moveaxis(weight, -1, 2), intercept, status, dropped, cond


def apply(weight, intercept, preds, groups=None):
    """weight (G, H, M, I), intercept (G, H, I) (broadcastable), preds M arrays (S, H, I) -> (S, H, I) float64: the intercept
    plus the members in ascending m; NaN rows for ids outside [0, G)."""
    S = preds[0].shape[0]
    G, H, M, I = weight.shape[0], preds[0].shape[1], len(preds), preds[0].shape[2]
    weight = np.broadcast_to(weight, (G, H, M, I))
    intercept = np.broadcast_to(intercept, (G, H, I))
    ids = np.zeros(S, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    out = np.full((S, H, I), np.nan)
    with np.errstate(invalid="ignore"):
        for s in range(S):
            g = ids[s]
            if not 0 <= g < G:
                continue
            acc = intercept[g].copy()
            for m in range(M):
                acc = acc + weight[g, :, m, :] * np.broadcast_to(preds[m], (S, H, I))[s].astype(np.float64)
            out[s] = acc
    return out


def members_and_truth(seed, S, H, I, M, coef=None, noise=0.5):
    """M well-conditioned N(0, 1) members with distinct means and a truth that is an affine blend of them plus noise,
    float32 (S, H, I)."""
    rng = np.random.default_rng(seed)
    preds = [(rng.standard_normal((S, H, I)) + 0.25 * m).astype(np.float32) for m in range(M)]
    coef = rng.uniform(-1.0, 1.0, M) if coef is None else np.asarray(coef)
    y = 0.75 + sum(c * p.astype(np.float64) for c, p in zip(coef, preds)) + noise * rng.standard_normal((S, H, I))
    return preds, y.astype(np.float32)


# ------------------------------------------------------------------------------------ the 12-node world
def window_members(y, L_in, H, starts, kinds, period=12):
    """The window baselines of tecmollm.evaluate on a (T, N) float32 series that is its own input channel, as float32
    (B, H, N) arrays: "mean" (the float32 mean of the window, rounded from float64), "last", "periodic"."""
    starts = np.asarray(starts, dtype=np.int64)
    out = {}
    for kind in kinds:
        if kind == "mean":
            v = np.stack([y[a:a + L_in].astype(np.float64).mean(axis=0) for a in starts]).astype(np.float32)
            out[kind] = np.repeat(v[:, None, :], H, axis=1)
        elif kind == "last":
            out[kind] = np.repeat(y[starts + L_in - 1][:, None, :], H, axis=1)
        else:
            out[kind] = np.stack([y[starts + L_in - period + (h % period)] for h in range(H)], axis=1)
    return out


def window_targets(y, L_in, H, starts):
    starts = np.asarray(starts, dtype=np.int64)
    return np.stack([y[starts + L_in + h] for h in range(H)], axis=1)       # (B, H, N)


def rmse(p, t):
    return float(np.sqrt(np.mean((np.asarray(p, dtype=np.float64) - np.asarray(t, dtype=np.float64)) ** 2)))


def held_out(y, kinds=("mean", "last", "periodic"), L_in=48, H=12, ridge=0.0):
    """Fit on the first two thirds of the stride-1 windows of `y`, blend the last third.  Returns a dict: the held-out RMSE of
    the blend ("combination") and of every member, `dropped` (1, H, N), and the in-sample members, truth and blend."""
    S = y.shape[0] - L_in - H + 1
    n_fit = 2 * S // 3
    fit, test = np.arange(n_fit), np.arange(n_fit, S)
    mem_fit, mem_test = window_members(y, L_in, H, fit, kinds), window_members(y, L_in, H, test, kinds)
    t_fit, t_test = window_targets(y, L_in, H, fit), window_targets(y, L_in, H, test)
    st = moments([mem_fit[k] for k in kinds], t_fit)
    weight, intercept, status, dropped, _ = solve(st, ridge)
    blend = apply(weight, intercept, [mem_test[k] for k in kinds]).astype(np.float32)
    out = {k: rmse(mem_test[k], t_test) for k in kinds}
    out["combination"] = rmse(blend, t_test)
    out.update(dropped=dropped, status=status, weight=weight, intercept=intercept, members_fit=mem_fit, truth_fit=t_fit,
               blend_fit=apply(weight, intercept, [mem_fit[k] for k in kinds]).astype(np.float32))
    return out


def world_series():
    return LR.synthetic(600, 12, 1, seasonal=True)
