"""float64 numpy restatement of the field scores (tecm_field_scores, include/tecmollm.h (3m)), shared by
tests/test_host_fields.py and tests/test_gpu_fields.py, and the generator of the coherent / shuffled ensembles that motivate
them.

The value pipeline is the float32 one of the other statistics (tests/ensemble_ref.values); everything after it is float64,
straight from the definitions: norms over the nodes, pair terms over the strict upper triangle of the class matrix.  Next
to every sum it returns what the error bars of tests/test_gpu_fields.py are made of: the norms that enter an energy sum
(all non-negative), and for the variogram sums the worst-case float32 rounding bound of the per-pair term,

    delta = (K + 4) * 2^-23 * (v_o + v_e) per pair,   sum (2 |e| + delta) delta  for sum e^2,
                                                      sum (2 + delta) delta      for sum v_o and sum v_e.

Cost O(S * H * K * I^2): pair a large K with H = 1."""
import numpy as np

from tests import ensemble_ref as ER

F32, F64 = np.float32, np.float64
EXCLUDED = 255


def f_order(d, order):
    if order == 0.5:
        return np.sqrt(d)
    if order == 1:
        return d
    assert order == 2
    return d * d


def per_sample(members, true, scaler=None, pair_class=None, NB=0, order=0.5):
    """Scaled float32 members (K, S, H, I) and truth (S, H, I) -> dict of float64 arrays:
    es (S, H, 3) = [A, D, E];  vs (S, H, NB, 4) = [pairs, sum e^2, sum v_o, sum v_e];  vs_bound (S, H, NB, 3), the error
    bars of the last three."""
    K, S, H, I = members.shape
    x32, y32 = ER.values(members, true, scaler)
    x, y = x32.astype(F64), y32.astype(F64)
    es = np.zeros((S, H, 3))
    for k in range(K):
        es[..., 0] += np.sqrt(((x[k] - y) ** 2).sum(axis=-1))
        for k2 in range(k + 1, K):
            es[..., 1] += np.sqrt(((x[k] - x[k2]) ** 2).sum(axis=-1))
    es[..., 0] /= F64(K)
    mu = np.zeros_like(y)
    for k in range(K):
        mu = mu + x[k]
    es[..., 2] = np.sqrt(((mu / F64(K) - y) ** 2).sum(axis=-1))
    vs, bound = np.zeros((S, H, NB, 4)), np.zeros((S, H, NB, 3))
    if NB:
        pc = np.asarray(pair_class)
        assert pc.shape == (I, I) and pc.dtype == np.uint8
        iu, ju = np.triu_indices(I, k=1)
        cls = pc[iu, ju]
        keep = cls < NB
        iu, ju, cls = iu[keep], ju[keep], cls[keep]
        sel = [cls == c for c in range(NB)]
        eps = F64(K + 4) * 2.0 ** -23
        for s in range(S):
            for h in range(H):
                vo = f_order(np.abs(y[s, h, iu] - y[s, h, ju]), order)
                ve = np.zeros_like(vo)
                for k in range(K):
                    ve = ve + f_order(np.abs(x[k, s, h, iu] - x[k, s, h, ju]), order)
                ve = ve / F64(K)
                e = vo - ve
                delta = eps * (vo + ve)
                for c in range(NB):
                    m = sel[c]
                    vs[s, h, c] = [m.sum(), (e[m] ** 2).sum(), vo[m].sum(), ve[m].sum()]
                    bound[s, h, c] = [((2 * np.abs(e[m]) + delta[m]) * delta[m]).sum(), ((2 + delta[m]) * delta[m]).sum(),
                                      ((2 + delta[m]) * delta[m]).sum()]
    return {"es": es, "vs": vs, "vs_bound": bound}


def accumulate(es_stats, es_mags, vs_stats, vs_bound, members, true, groups=None, scaler=None, pair_class=None, order=0.5):
    """One update into es_stats / es_mags (G, H, 4) -- [n, sum A, sum D, sum E] and the same sums again as the magnitudes of
    the energy error bar (every term is non-negative) -- and vs_stats (G, H, NB, 5) = [n, sum pairs, sum e^2, sum v_o, sum v_e]
    with vs_bound (G, H, NB, 3), samples in ascending s.  A sample whose id is outside [0, G) is skipped.  Returns the
    per-sample dict."""
    G, NB = es_stats.shape[0], vs_stats.shape[2]
    q = per_sample(members, true, scaler, pair_class, NB, order)
    for s in range(true.shape[0]):
        g = 0 if groups is None else int(groups[s])
        if not 0 <= g < G:
            continue
        es_stats[g, :, 0] += 1
        es_stats[g, :, 1:] += q["es"][s]
        es_mags[g, :, 1:] += q["es"][s]
        vs_stats[g, :, :, 0] += 1
        vs_stats[g, :, :, 1:] += q["vs"][s]
        vs_bound[g] += q["vs_bound"][s]
    return q


def energy_bar(I, K, S, mags):
    """|kernel - ref| <= (I + K^2 + S + 16) * 2^-53 * (sum of the norms that enter): any order of the additions."""
    return (I + K * K + S + 16) * 2.0 ** -53 * mags


# ------------------------------------------------------------------------------------ coherent against shuffled members
def grid_distances(rows=9, cols=13, lat0=30.0, lon0=100.0):
    """Haversine distances (km) of a rows x cols one-degree grid, node = row * cols + col."""
    la, lo = np.meshgrid(np.radians(lat0 + np.arange(rows)), np.radians(lon0 + np.arange(cols)), indexing="ij")
    la, lo = la.ravel(), lo.ravel()
    a = np.sin((la[None] - la[:, None]) / 2) ** 2 + np.cos(la[:, None]) * np.cos(la[None]) * np.sin((lo[None] - lo[:, None]) / 2) ** 2
    return 2 * np.arcsin(np.sqrt(a)) * 6371.0


def coherent_and_shuffled(seed, K=8, S=6, H=3, rows=9, cols=13, range_km=500.0):
    """A Gaussian field with exponential covariance exp(-d / range_km) on the grid: truth (S, H, I) and K members (K, S, H, I)
    drawn alike, float32 in scaled units; and the same members permuted independently at every (s, h, node).  Returns
    (members, shuffled, truth, distances)."""
    rng = np.random.default_rng(seed)
    d = grid_distances(rows, cols)
    L = np.linalg.cholesky(np.exp(-d / range_km) + 1e-10 * np.eye(d.shape[0]))
    draw = (rng.standard_normal((K + 1, S, H, d.shape[0])) @ L.T).astype(F32)
    members, truth = draw[:K], draw[K]
    perm = np.argsort(rng.random(members.shape), axis=0)
    return members, np.take_along_axis(members, perm, axis=0), truth, d
