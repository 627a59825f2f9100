"""numpy statements of the ensemble statistics (tecm_ensemble_stats), shared by tests/test_host_ensemble.py and
tests/test_gpu_ensemble.py.

`per_sample` / `accumulate` restate the kernel: the value pipeline in float32 (tests/error_maps_ref.pipeline), everything
after it in float64, every sum over members in ascending SORTED order one term at a time, samples added in ascending s.
`independent` defines the same quantities another way -- the CRPS from the O(K^2) pairwise differences, coverage by
direct interval membership, the rank by counting -- and knows nothing of the sorted-order identities."""
import numpy as np

from tests.error_maps_ref import pipeline

F32, F64 = np.float32, np.float64
STATS = 9          # count, sum y, sum mu, sum (mu-y)^2, sum |mu-y|, sum var, sum A, sum D, sum width


def values(members, true, scaler=None):
    """Scaled float32 members (K, ...) and truth (...) -> (x (K, ...), y (...)) float32 in physical units."""
    K = members.shape[0]
    y, _ = pipeline(np.zeros_like(true, dtype=F32), true, scaler)
    x = np.stack([pipeline(members[k], true, scaler)[1] for k in range(K)])
    return x, y


def per_sample(members, true, scaler=None, trim=0):
    """Every per-(sample, horizon, node) quantity of the kernel, from scaled float32 members (K, S, H, I) and truth
    (S, H, I): a dict of float64 arrays (S, H, I) -- mu, var, A, D, width, rank (int64), lo, hi (float32), mean_raw
    (float64: the mean over k ascending of the raw members, non-finite -> 0) -- and `D_mag`, the sum of |terms| of D."""
    K, m = members.shape[0], int(trim)
    assert K >= 2 and 0 <= 2 * m < K - 1
    x, y32 = values(members, true, scaler)
    y = y32.astype(F64)
    lt = (x < y32[None]).sum(axis=0)
    eq = (x == y32[None]).sum(axis=0)
    rank = (lt + eq // 2).astype(np.int64)
    xs = np.sort(x, axis=0).astype(F64)
    total = np.zeros_like(y)
    for j in range(K):
        total = total + xs[j]
    mu = total / F64(K)
    ss, sa, D, D_mag = np.zeros_like(y), np.zeros_like(y), np.zeros_like(y), np.zeros_like(y)
    for j in range(K):
        d = xs[j] - mu
        ss = ss + d * d
        sa = sa + np.abs(xs[j] - y)
        c = F64(2 * (j + 1) - K - 1)
        D = D + c * xs[j]
        D_mag = D_mag + np.abs(c * xs[j])
    raw = np.zeros_like(y)
    with np.errstate(invalid="ignore"):
        finite = np.where(np.isfinite(members), members, F32(0)).astype(F64)
    for k in range(K):
        raw = raw + finite[k]
    lo, hi = xs[m].astype(F32), xs[K - 1 - m].astype(F32)
    return {"y": y, "mu": mu, "var": ss / (F64(K) - 1.0), "A": sa / F64(K), "D": D, "D_mag": D_mag,
            "width": hi.astype(F64) - lo.astype(F64), "rank": rank, "lo": lo, "hi": hi, "mean_raw": raw / F64(K)}


def terms(q):
    """(9, S, H, I) float64: what each sample adds to the nine statistics, and the magnitudes behind the error bar."""
    e = q["mu"] - q["y"]
    t = np.stack([np.ones_like(e), q["y"], q["mu"], e * e, np.abs(e), q["var"], q["A"], q["D"], q["width"]])
    mags = np.abs(t)
    mags[7] = q["D_mag"]
    return t, mags


def accumulate(stats, mags, hist, members, true, groups=None, scaler=None, trim=0):
    """One update into stats / mags (G, H, 9, I) float64 and hist (G, H, K+1, I) int64, samples in ascending s as the
    kernel adds them.  A sample whose id is outside [0, G) is skipped.  Returns the per-sample dict."""
    q = per_sample(members, true, scaler, trim)
    t, mg = terms(q)
    G, K = stats.shape[0], members.shape[0]
    H, I = true.shape[1], true.shape[2]
    hh, ii = np.meshgrid(np.arange(H), np.arange(I), indexing="ij")
    for s in range(true.shape[0]):
        g = 0 if groups is None else int(groups[s])
        if not 0 <= g < G:
            continue
        stats[g] += t[:, s].transpose(1, 0, 2)
        mags[g] += mg[:, s].transpose(1, 0, 2)
        assert q["rank"][s].min() >= 0 and q["rank"][s].max() <= K
        hist[g][hh, q["rank"][s], ii] += 1
    return q


def independent(members, true, scaler=None, trim=0):
    """The same per-sample quantities from their definitions: crps = mean_k |x_k - y| - (1 / 2K^2) sum_{a,b} |x_a - x_b|,
    fair_crps with 1 / (2 K (K - 1)), D = sum over unordered pairs of |x_a - x_b|, var = np.var(ddof=1), mu = np.mean,
    inside = lo < y < hi with lo / hi the (m+1)-th smallest / largest, rank by counting members below y plus half the ties
    (rounded down)."""
    K, m = members.shape[0], int(trim)
    x, y32 = values(members, true, scaler)
    x, y = x.astype(F64), y32.astype(F64)
    pair = np.zeros_like(y)
    for a in range(K):
        for b in range(a + 1, K):
            pair += np.abs(x[a] - x[b])
    A = np.abs(x - y[None]).mean(axis=0)
    part = np.partition(x, (m, K - 1 - m), axis=0)
    lo, hi = part[m], part[K - 1 - m]
    rank = np.zeros(y.shape, dtype=np.int64)
    ties = np.zeros(y.shape, dtype=np.int64)
    for k in range(K):
        rank += x[k] < y
        ties += x[k] == y
    return {"mu": x.mean(axis=0), "var": x.var(axis=0, ddof=1), "A": A, "D": pair, "crps": A - pair / K ** 2,
            "fair_crps": A - pair / (K * (K - 1)), "width": hi - lo, "inside": (lo < y) & (y < hi),
            "rank": rank + ties // 2, "ties": ties}
