"""float64 numpy restatement of the subset seasonal ARMA that `SarimaBaseline` fits and forecasts on the device
(include/tecmollm.h (7)): differencing, sample autocovariances, Levinson-Durbin, the Hannan-Rissanen regression, the
invertibility check and the window forecast.  Vectorised over nodes, plain loops over time; written from the formulas, not
from the kernels, and summed in numpy's own order."""
import numpy as np

DEGENERATE, NONFINITE, MA_DROPPED = 1, 2, 4
MAX_K, MAX_LAG, MAX_LONG_AR, MAX_OFFSET = 12, 32, 64, 64


class Model:
    def __init__(self, order=(1, 1, 1), seasonal_order=(1, 1, 1, 12), long_ar=None):
        p, d, q = order
        P, D, Q, s = seasonal_order
        if d not in (0, 1) or D not in (0, 1) or min(p, q, P, Q) < 0 or ((P or Q or D) and s < 1):
            raise ValueError("outside the served range")
        self.d, self.D, self.s = d, D, s
        self.ar = sorted({i + s * j for i in range(p + 1) for j in range(P + 1)} - {0})
        self.ma = sorted({i + s * j for i in range(q + 1) for j in range(Q + 1)} - {0})
        self.K = len(self.ar) + len(self.ma)
        if not 1 <= self.K <= MAX_K:
            raise ValueError("K outside [1, 12]")
        self.lmax = max(self.ar + self.ma)
        self.o = d + s * D
        if self.lmax > MAX_LAG or self.o > MAX_OFFSET:
            raise ValueError("lag or offset too large")
        self.m = min(max(2 * self.lmax, 8), MAX_LONG_AR) if long_ar is None else int(long_ar)
        if not self.lmax <= self.m <= MAX_LONG_AR:
            raise ValueError("long_ar outside [Lmax, 64]")


def difference(y, mo):
    """(T, N) -> (T - o, N) float64: w_u = (y_t - y_{t-1}) - (y_{t-s} - y_{t-s-1}), t = u + o."""
    y = np.asarray(y).astype(np.float64)
    t = np.arange(mo.o, y.shape[0])
    w = y[t]
    if mo.d:
        w = w - y[t - 1]
    if mo.D:
        q = y[t - mo.s]
        if mo.d:
            q = q - y[t - mo.s - 1]
        w = w - q
    return w


def autocov_terms(w, m):
    """gamma (N, m + 1) and the sum of the absolute values of the terms of each (for the summation-order tolerance)."""
    n, N = w.shape
    g, mag = np.zeros((N, m + 1)), np.zeros((N, m + 1))
    for k in range(min(m, n - 1) + 1 if n > 0 else 0):
        prod = w[k:] * w[:n - k]
        g[:, k], mag[:, k] = prod.sum(axis=0) / n, np.abs(prod).sum(axis=0) / n
    return g, mag


def levinson(g):
    """(N, m + 1) autocovariances -> ((N, m) long-AR coefficients, (N,) ok)."""
    N, m = g.shape[0], g.shape[1] - 1
    phi, var, ok = np.zeros((N, m)), g[:, 0].copy(), np.ones(N, dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(1, m + 1):
            prev = phi[:, :i - 1]                                            # phi_1 .. phi_{i-1}
            r = g[:, i] - (prev * g[:, 1:i][:, ::-1]).sum(axis=1)           # - sum_j phi_j gamma_{i-j}
            kap = r / var
            new = phi.copy()
            new[:, :i - 1] = prev - kap[:, None] * prev[:, ::-1]
            new[:, i - 1] = kap
            phi = np.where(ok[:, None], new, phi)
            var = np.where(ok, var * (1.0 - kap * kap), var)
            ok &= var > 0.0
    return phi, ok


def innovations(w, phi):
    """e_u = w_u - sum_{i <= m} phi_i w_{u-i} for u >= m (rows below m are left NaN)."""
    n, m = w.shape[0], phi.shape[1]
    e = np.full_like(w, np.nan)
    if n > m:
        e[m:] = w[m:]
        for i in range(1, m + 1):
            e[m:] -= phi[:, i - 1] * w[m - i:n - i]
    return e


def regressors(w, e, mo):
    """(rows, N, K) z_u and (rows, N) w_u for u = m + Lmax .. n - 1."""
    n = w.shape[0]
    u = np.arange(mo.m + mo.lmax, n)
    if u.size == 0:
        return np.zeros((0, w.shape[1], mo.K)), np.zeros((0, w.shape[1]))
    z = np.stack([w[u - a] for a in mo.ar] + [e[u - b] for b in mo.ma], axis=2)
    return z, w[u]


def cholesky_solve(G, r, ke):
    """Solves the leading ke x ke block per node; ok False where a pivot <= 1e-12 G_kk."""
    N = G.shape[0]
    coef, ok = np.zeros((N, G.shape[1])), np.ones(N, dtype=bool)
    for i in range(N):
        A, L = G[i, :ke, :ke], np.zeros((ke, ke))
        with np.errstate(all="ignore"):
            for k in range(ke):
                p = A[k, k] - (L[k, :k] ** 2).sum()
                if not p > 1e-12 * A[k, k]:
                    ok[i] = False
                    break
                L[k, k] = np.sqrt(p)
                L[k + 1:, k] = (A[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
        if ok[i] and ke:
            y = np.linalg.solve(L, r[i, :ke])
            coef[i, :ke] = np.linalg.solve(L.T, y)
    return coef, ok


def fit(y, mo, use_ma=None):
    """The whole fit of a (T, N) series.  Returns a dict: autocov, autocov_mag, gram (N, K, K+1), gram_mag, wss, coef, sigma2,
    status, cond_gram, cond_toeplitz.  `use_ma` (N) of 0 / 1: nodes with 0 are solved as pure AR and get MA_DROPPED."""
    y = np.asarray(y)
    N, K, m = y.shape[1], mo.K, mo.m
    status = np.zeros(N, dtype=np.int32)
    with np.errstate(all="ignore"):
        w = difference(y, mo)
        n = w.shape[0]
        g, gmag = autocov_terms(w, m)
        status[~np.isfinite(g[:, 0])] = NONFINITE
        status[(status == 0) & (~(g[:, 0] > 0.0) | (n < m + mo.lmax + 2 * K))] = DEGENERATE
        phi, ok = levinson(np.where((status == 0)[:, None], g, 1.0 * (np.arange(m + 1) == 0)[None, :]))
        status[(status == 0) & ~ok] = DEGENERATE
        phi[status != 0] = 0.0
        e = innovations(w, phi)
        z, wu = regressors(w, e, mo)
        rows = z.shape[0]
        G = np.einsum("unj,unk->njk", z, z)
        r = np.einsum("unj,un->nj", z, wu)
        gram = np.concatenate([G, r[:, :, None]], axis=2)
        gram_mag = np.concatenate([np.einsum("unj,unk->njk", np.abs(z), np.abs(z)),
                                   np.einsum("unj,un->nj", np.abs(z), np.abs(wu))[:, :, None]], axis=2)
        wss = (wu * wu).sum(axis=0)
        coef, sigma2 = np.zeros((N, K)), np.zeros(N)
        full = np.ones(N, dtype=bool) if use_ma is None else np.asarray(use_ma).astype(bool)
        for sel, ke in ((full, K), (~full, len(mo.ar))):
            idx = np.flatnonzero(sel & (status == 0))
            if idx.size == 0:
                continue
            c, ok = cholesky_solve(G[idx], r[idx], ke)
            coef[idx] = c
            res = wu[:, idx] - np.einsum("unj,nj->un", z[:, idx], c)
            sigma2[idx] = (res * res).sum(axis=0) / rows
            status[idx[~ok]] = DEGENERATE
        deg, bad = (status & DEGENERATE) != 0, (status & NONFINITE) != 0
        coef[deg], sigma2[deg] = 0.0, g[deg, 0]
        coef[bad], sigma2[bad] = np.nan, np.nan
        if use_ma is not None and len(mo.ma):
            status[~full] |= MA_DROPPED
        good = np.flatnonzero(status == 0)
        cond_gram = max([np.linalg.cond(G[i]) for i in good], default=0.0)
        cond_toep = max([np.linalg.cond(g[i, np.abs(np.subtract.outer(np.arange(m), np.arange(m)))]) for i in good], default=0.0)
    return dict(autocov=g, autocov_mag=gmag, gram=gram, gram_mag=gram_mag, wss=wss, coef=coef, sigma2=sigma2, status=status,
                cond_gram=cond_gram, cond_toeplitz=cond_toep, rows=rows)


def ma_invertible(theta, ma_lags):
    """(N, n_ma) -> (N,) bool: every root of 1 + sum theta_b z^b outside the unit circle (np.roots per node)."""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    out = np.ones(theta.shape[0], dtype=bool)
    for i, th in enumerate(theta):
        if not len(ma_lags) or not np.isfinite(th).all():
            continue
        poly = np.zeros(max(ma_lags) + 1)
        poly[0] = 1.0
        poly[np.asarray(ma_lags)] = th
        roots = np.roots(poly[::-1])                      # highest power first
        out[i] = bool((np.abs(roots) > 1.0).all())
    return out


def forecast(yw, coef, mo, L_out):
    """(L_in, N) window, (N, K) coefficients -> (L_out, N) float64 forecasts (round to float32 to compare with the device)."""
    yw = np.asarray(yw).astype(np.float64)
    L_in, N = yw.shape
    if L_in < mo.o + mo.lmax + 1:
        raise ValueError("window too short")
    coef = np.asarray(coef, dtype=np.float64)
    na = len(mo.ar)
    w = difference(yw, mo)
    nw = w.shape[0]
    w = np.concatenate([w, np.zeros((L_out, N))])
    e = np.zeros_like(w)
    y = np.concatenate([yw, np.zeros((L_out, N))])
    with np.errstate(all="ignore"):
        def arma(u):
            acc = np.zeros(N)
            for j, a in enumerate(mo.ar):
                acc = acc + coef[:, j] * w[u - a]
            for j, b in enumerate(mo.ma):
                acc = acc + coef[:, na + j] * e[u - b]
            return acc
        for u in range(mo.lmax, nw):
            e[u] = w[u] - arma(u)
        for h in range(L_out):
            u, t = nw + h, L_in + h
            w[u] = arma(u)
            v = w[u].copy()
            if mo.d:
                v = v + y[t - 1]
            if mo.D:
                q = y[t - mo.s]
                if mo.d:
                    q = q - y[t - mo.s - 1]
                v = v + q
            y[t] = v
    return y[L_in:]


def synthetic(T, N, seed, amp=20.0):
    """(T, N) float32 TEC-like series: diurnal shape x slow amplitude + AR(1) noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    phase = rng.uniform(0, 2 * np.pi, N)[None, :]
    diurnal = 1.0 + 0.6 * np.sin(2 * np.pi * t / 12 + phase) + 0.2 * np.sin(4 * np.pi * t / 12 + 2 * phase)
    slow = amp * (1.0 + 0.3 * np.sin(2 * np.pi * t / 327.0 + phase))
    noise = np.zeros((T, N))
    eps = rng.standard_normal((T, N))
    for i in range(1, T):
        noise[i] = 0.7 * noise[i - 1] + eps[i]
    return (diurnal * slow + 1.5 * noise).astype(np.float32)
