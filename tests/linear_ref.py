"""float64 numpy restatement of the ridge regression `LinearBaseline` fits and forecasts on the device
(include/tecmollm.h (9)): the design matrix, the normal equations as a sequential loop over the windows in ascending
order (the order the device promises, for the bit-for-bit check), the ridge solve by `np.linalg.solve`, the status
rules and the forecast.  Vectorised over nodes; written from the formulas, not from the kernels."""
import numpy as np

DEGENERATE, NONFINITE = 1, 2
MAX_P, MAX_H, MAX_LAG, MAX_CHANNELS = 64, 32, 512, 8


def default_pairs(L_in, channel=0, lags=None, exog=()):
    lags = range(1, min(L_in, 48) + 1) if lags is None else lags
    return [(channel, int(l)) for l in lags] + [(int(c), int(l)) for c, l in exog]


def synthetic(T, N, seed, seasonal=False, phi=0.5):
    """(T, N) float32: a stationary AR(1) with coefficient phi and unit variance per node, optionally plus
    sin(2 pi t / 12 + phase_n)."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((T + 50, N)) * np.sqrt(1.0 - phi * phi)
    y = np.zeros((T + 50, N))
    y[0] = rng.standard_normal(N)
    for t in range(1, T + 50):
        y[t] = phi * y[t - 1] + e[t]
    y = y[50:]
    if seasonal:
        y = y + np.sin(2.0 * np.pi * np.arange(T)[:, None] / 12.0 + rng.uniform(0.0, 2.0 * np.pi, N)[None, :])
    return y.astype(np.float32)


def design(X, pairs, L_in, starts):
    """X (T, N, C) -> z (B, N, P) float64: z[b, n] = [1, X[a + L_in - l, n, c] for (c, l) in pairs], a = starts[b]."""
    X = np.asarray(X)
    starts = np.asarray(starts, dtype=np.int64)
    z = np.ones((len(starts), X.shape[1], len(pairs) + 1))
    for p, (c, l) in enumerate(pairs, start=1):
        z[:, :, p] = X[starts + L_in - l, :, c].astype(np.float64)
    return z


def targets(ys, L_in, H, starts):
    """ys (Ty, N) -> y (B, N, H) float64: y[b, n, h] = ys[a + L_in + h, n]."""
    ys = np.asarray(ys)
    starts = np.asarray(starts, dtype=np.int64)
    return np.stack([ys[starts + L_in + h].astype(np.float64) for h in range(H)], axis=2)


def gram_sequential(X, ys, pairs, L_in, H, first, step, count, snapshots=()):
    """(N, P, P + H) = [G | R], every entry one running float64 sum over the windows in ascending order.  With `snapshots`
    (window counts <= count) a dict {count: the sums after that many windows} instead: a shorter fit is a prefix."""
    N, P = np.asarray(X).shape[1], len(pairs) + 1
    out, kept = np.zeros((N, P, P + H)), {}
    for i in range(count):
        a = first + i * step
        z = design(X, pairs, L_in, [a])[0]
        v = np.concatenate([z, targets(ys, L_in, H, [a])[0]], axis=1)
        out += z[:, :, None] * v[:, None, :]
        if i + 1 in snapshots:
            kept[i + 1] = out.copy()
    return kept if snapshots else out


def gram(X, ys, pairs, L_in, H, first, step, count):
    """The same sums by matrix products (numpy's order): for everything that is not the bit-for-bit check."""
    starts = first + step * np.arange(count)
    z = design(X, pairs, L_in, starts)
    v = np.concatenate([z, targets(ys, L_in, H, starts)], axis=2)
    return np.einsum("bnp,bnq->npq", z, v)


def pooled(g):
    """The nodes' arrays added in ascending node order."""
    out = np.zeros(g.shape[1:])
    for n in range(g.shape[0]):
        out += g[n]
    return out


def ridge_matrix(g, alpha):
    P = g.shape[1]
    D = np.eye(P)
    D[0, 0] = 0.0
    return g[:, :, :P] + alpha * D


def solve(g, alpha):
    """g (N, P, P + H) -> (coef (N, P, H), status (N), cond (N)).  NONFINITE: any non-finite entry (NaN coefficients).
    DEGENERATE: a Cholesky pivot <= 1e-12 x its diagonal entry of G + alpha D (the intercept-only model
    coef[0, h] = R[0, h] / G[0, 0])."""
    N, P = g.shape[0], g.shape[1]
    H = g.shape[2] - P
    coef, status, cond = np.zeros((N, P, H)), np.zeros(N, dtype=np.int32), np.full(N, np.inf)
    A = ridge_matrix(np.nan_to_num(g), alpha)
    for n in range(N):
        if not np.isfinite(g[n]).all():
            coef[n], status[n] = np.nan, NONFINITE
            continue
        L = np.zeros((P, P))
        ok = True
        for k in range(P):
            piv = A[n, k, k] - L[k, :k] @ L[k, :k]
            if not piv > 1e-12 * A[n, k, k]:
                ok = False
                break
            L[k, k] = np.sqrt(piv)
            L[k + 1:, k] = (A[n, k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
        if not ok:
            status[n] = DEGENERATE
            coef[n, 0] = g[n, 0, P:] / g[n, 0, 0]
            continue
        coef[n] = np.linalg.solve(A[n], g[n, :, P:])
        cond[n] = np.linalg.cond(A[n])
    return coef, status, cond


def forecast(X, pairs, L_in, starts, coef):
    """coef (N or 1, P, H) -> (B, H, N) float64: z^T W_n."""
    z = design(X, pairs, L_in, starts)
    W = np.broadcast_to(coef, (z.shape[1],) + coef.shape[1:])
    return np.einsum("bnp,nph->bhn", z, W)


def fit(X, ys, pairs, L_in, H, first, step, count, alpha, pool=False):
    g = gram(X, ys, pairs, L_in, H, first, step, count)
    return solve(pooled(g)[None] if pool else g, alpha)


def rmse(pred, truth):
    return float(np.sqrt(np.mean((np.asarray(pred, dtype=np.float64) - np.asarray(truth, dtype=np.float64)) ** 2)))


def held_out_scores(y, L_in=48, H=12, alpha=0.0):
    """The sanity recipe on a (T, N) series that is both the input channel and the target: fit on the first two thirds of
    the stride-1 windows, score the last third.  {"linear", "mean", "last"}: RMSE over every window, horizon and node."""
    X = y[:, :, None]
    S = y.shape[0] - L_in - H + 1
    n_fit = 2 * S // 3
    pairs = default_pairs(L_in)
    coef, status, _ = fit(X, y, pairs, L_in, H, 0, 1, n_fit, alpha)
    assert (status == 0).all()
    test = np.arange(n_fit, S)
    truth = targets(y, L_in, H, test).transpose(0, 2, 1)                    # (B, H, N)
    z = design(X, pairs, L_in, test)[:, :, 1:]                              # (B, N, lags), lag 1 first
    mean = np.repeat(z.mean(axis=2)[:, None, :], H, axis=1)
    last = np.repeat(z[:, :, 0][:, None, :], H, axis=1)
    return {"linear": rmse(forecast(X, pairs, L_in, test, coef), truth), "mean": rmse(mean, truth), "last": rmse(last, truth)}
