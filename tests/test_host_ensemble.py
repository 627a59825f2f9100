"""CPU tests of the ensemble scores' host side: the ordered restatement of the kernel (tests/ensemble_ref.py) against
independent definitions and closed forms, a calibrated synthetic ensemble, the numpy derivation under `EnsembleMetrics`,
`member_seed`, `dropout_seed`, the files, and the entry point's argument checks through the C ABI (no device call is
reached)."""
import csv
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import ensemble_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALER = (21.5, 9.25)


def _members(K, S, H, I, rng, scaler, ties):
    m = (rng.standard_normal((K, S, H, I)) * 2.5).astype(np.float32)
    t = (rng.standard_normal((S, H, I)) * 2.5).astype(np.float32)
    if ties:
        # members far below / above the clip bounds [0, 200] TECU: equal after the clip; truths copied from a member
        m[rng.random(m.shape) < 0.25] = np.float32(-30.0)
        m[rng.random(m.shape) < 0.15] = np.float32(+40.0)
        copy = rng.random(t.shape) < 0.3
        t[copy] = m[rng.integers(K)][copy]
        t[0, 0, 0], m[0, 0, 0, 0], m[1, 0, 0, 0] = np.nan, np.inf, -np.inf
    return m, t


@pytest.mark.parametrize("K", [2, 3, 8, 17, 64])
@pytest.mark.parametrize("ties", [False, True])
def test_the_restatement_agrees_with_the_independent_definitions(K, ties):
    rng = np.random.default_rng(100 * K + ties)
    scaler = SCALER if ties else None
    for trim in sorted({0, (K - 2) // 2}):
        m, t = _members(K, 4, 3, 7, rng, scaler, ties)
        q, ind = ER.per_sample(m, t, scaler, trim), ER.independent(m, t, scaler, trim)
        scale = np.abs(ER.values(m, t, scaler)[0]).max() + 1.0
        for k in ("mu", "var", "A", "D", "width"):
            np.testing.assert_allclose(q[k], ind[k], rtol=0, atol=1e-11 * scale * scale * K, err_msg=f"{k} K={K} trim={trim}")
        crps, fair = q["A"] - q["D"] / K ** 2, q["A"] - q["D"] / (K * (K - 1))
        np.testing.assert_allclose(crps, ind["crps"], rtol=0, atol=1e-11 * scale)
        np.testing.assert_allclose(fair, ind["fair_crps"], rtol=0, atol=1e-11 * scale)
        assert (crps >= -1e-11 * scale).all()
        assert np.array_equal(q["rank"], ind["rank"]) and q["rank"].min() >= 0 and q["rank"].max() <= K
        # coverage: the rank lies in [m + 1, K - m - 1] exactly when the truth lies strictly inside [x_(1+m), x_(K-m)]
        # (without ties; with them the mid-rank rule decides, which the rank comparison above covers)
        clean = ind["ties"] == 0
        by_rank = (q["rank"] >= trim + 1) & (q["rank"] <= K - trim - 1)
        assert np.array_equal(by_rank[clean], ind["inside"][clean])
        if ties:
            x = ER.values(m, t, scaler)[0]
            assert (ind["ties"] > 0).any()
            assert ((x == 0).sum(axis=0) >= min(K, 2)).any() and ((x == 200).sum(axis=0) >= min(K, 2)).any()
        assert np.isfinite(q["mean_raw"]).all()


def test_closed_forms():
    m = np.array([0.0, 2.0], dtype=np.float32).reshape(2, 1, 1, 1)
    q = ER.per_sample(m, np.ones((1, 1, 1), dtype=np.float32))
    assert q["A"].item() == 1.0 and q["D"].item() == 2.0 and q["rank"].item() == 1
    assert (q["A"] - q["D"] / 4).item() == 0.5 and (q["A"] - q["D"] / 2).item() == 0.0
    assert q["mu"].item() == 1.0 and q["var"].item() == 2.0 and q["width"].item() == 2.0
    for K in (2, 3, 8, 17, 64):
        m = np.full((K, 1, 1, 1), 3.25, dtype=np.float32)
        q = ER.per_sample(m, np.full((1, 1, 1), 3.25, dtype=np.float32))
        assert q["A"].item() == 0.0 and q["D"].item() == 0.0 and q["var"].item() == 0.0
        assert q["rank"].item() == K // 2


def test_a_calibrated_synthetic_ensemble_scores_as_theory_says():
    """Members and truth iid N(0, 1), K = 8, 27 000 cells: the rank is uniform on 0..8, and the expectation of the fair
    CRPS is E|X - Y| - E|X - X'| / 2 = 1 / sqrt(pi)."""
    from src.evaluation.metrics import derive_ensemble
    K, S, H, I = 8, 10, 12, 225
    rng = np.random.default_rng(20240611)
    m = rng.standard_normal((K, S, H, I)).astype(np.float32)
    t = rng.standard_normal((S, H, I)).astype(np.float32)
    stats, mags, hist = np.zeros((1, H, 9, I)), np.zeros((1, H, 9, I)), np.zeros((1, H, K + 1, I), dtype=np.int64)
    q = ER.accumulate(stats, mags, hist, m, t)
    n = S * H * I
    assert n == 27000 and stats[0, :, 0].sum() == n
    pooled_hist = hist.sum(axis=(0, 1, 3))
    assert pooled_hist.sum() == n
    p = 1.0 / (K + 1)
    se = math.sqrt(p * (1 - p) / n)
    print("rank histogram / n:", pooled_hist / n, "5 se:", 5 * se)
    assert np.all(np.abs(pooled_hist / n - p) <= 5 * se)
    fair = q["A"] - q["D"] / (K * (K - 1))
    se_f = fair.std(ddof=1) / math.sqrt(n)
    print("mean fair CRPS", fair.mean(), "1/sqrt(pi)", 1 / math.sqrt(math.pi), "se", se_f)
    assert abs(fair.mean() - 1 / math.sqrt(math.pi)) <= 5 * se_f
    # the pooled derivation gives the same mean, and the ensemble CRPS is larger by mean(D) / (K^2 (K - 1))
    d = derive_ensemble(stats.sum(axis=(0, 1, 3)), pooled_hist, K, 1)
    assert abs(d["fair_crps"] - fair.mean()) < 1e-12 and d["crps"] > d["fair_crps"]
    assert abs(d["coverage"] - pooled_hist[2:7].sum() / n) < 1e-15 and abs(d["coverage"] - 5 / 9) <= 5 * math.sqrt(20 / 81 / n)
    assert abs(d["spread_skill"] - 1.0) < 0.03


def test_derive_ensemble_on_hand_built_statistics():
    from src.evaluation.metrics import ENSEMBLE_KEYS, EnsembleMetrics, derive_ensemble, nominal_coverage
    K, m = 4, 1
    #        count  Sy    Smu   Sse   Sae   Svar  SA    SD    Swidth
    row = [4.0, 40.0, 44.0, 16.0, 6.0, 36.0, 10.0, 32.0, 12.0]
    stats = np.array([row, [0.0] * 9])
    hist = np.array([[1, 0, 2, 1, 0], [0, 0, 0, 0, 0]])
    d = derive_ensemble(stats, hist, K, m)
    assert set(d) == set(ENSEMBLE_KEYS)
    want = {"count": 4.0, "crps": (10.0 - 32.0 / 16) / 4, "fair_crps": (10.0 - 32.0 / 12) / 4, "rmse_mean": 2.0,
            "mae_mean": 1.5, "bias_mean": 1.0, "spread": 3.0, "spread_skill": math.sqrt(5 / 4 * 9.0 / 4.0),
            "coverage": 0.5, "interval_width": 3.0}
    for k, v in want.items():
        assert d[k][0] == pytest.approx(v, rel=1e-15), k
        if k != "count":
            assert np.isnan(d[k][1]), k
    assert d["count"][1] == 0
    assert nominal_coverage(4, 1) == 1 / 5 and nominal_coverage(16, 1) == 13 / 17 and nominal_coverage(8, 0) == 7 / 9
    with pytest.raises(ValueError):
        derive_ensemble(stats, hist, 5, 1)
    with pytest.raises(ValueError):
        derive_ensemble(stats, hist, 4, 2)
    # the object: (G, H, 9, I) / (G, H, K+1, I) on the CPU, compute() from them
    em = EnsembleMetrics(2, 3, K, 2, None, m, device="cpu")
    assert em.stats.shape == (2, 2, 9, 3) and em.hist.shape == (2, 2, 5, 3) and em.hist.dtype == torch.int32
    em.stats[0, :, :, :] = torch.tensor(row, dtype=torch.float64).view(1, 9, 1)
    em.hist[0, :, :, :] = torch.tensor(hist[0], dtype=torch.int32).view(1, 5, 1)
    assert em.merge_() is em                                               # no process group: a no-op
    out = em.compute()
    assert set(out) == set(ENSEMBLE_KEYS) | {"nominal_coverage", "rank_histogram", "by_group"}
    assert out["nominal_coverage"] == 1 / 5
    for k, v in want.items():
        assert out[k].shape == (2, 2, 3)
        np.testing.assert_allclose(out[k][0], v, rtol=1e-15)
        assert np.isnan(out[k][1]).all() or k == "count"
    assert out["rank_histogram"].shape == (2, 2, 5) and out["rank_histogram"][0, 0].tolist() == [3, 0, 6, 3, 0]
    pooled = out["by_group"][0]
    assert pooled["crps_avg"] == pytest.approx(want["crps"]) and pooled["coverage_by_horizon"] == [0.5, 0.5]
    assert pooled["count_by_horizon"] == [12.0, 12.0] and np.isnan(out["by_group"][1]["crps_avg"])
    em.reset()
    assert float(em.stats.abs().sum()) == 0.0 and int(em.hist.sum()) == 0
    for bad in (dict(members=1), dict(members=65), dict(members=4, trim=2), dict(members=4, trim=-1)):
        with pytest.raises(ValueError):
            EnsembleMetrics(2, 3, num_groups=1, device="cpu", **bad)


def test_member_seed_is_pure_and_distinct():
    from tecmollm import member_seed, ops
    from tecmollm.ensemble import member_seed as again
    assert member_seed is again
    grid = {(c, k): member_seed(7, c, k) for c in range(64) for k in range(64)}
    assert len(set(grid.values())) == 64 * 64
    assert all(member_seed(7, c, k) == v for (c, k), v in grid.items())    # the same value on a second call
    assert all(isinstance(v, int) and 0 <= v < 1 << 64 for v in grid.values())
    assert member_seed(7, 3, 5) == ops.splitmix64((ops.splitmix64(7) + 3 * 256 + 5) & ((1 << 64) - 1))
    assert member_seed(8, 0, 0) != member_seed(7, 0, 0) and member_seed(-1, 0, 0) == member_seed((1 << 64) - 1, 0, 0)
    for bad in ((0, -1), (0, 256), (-1, 0), (1 << 56, 0)):
        with pytest.raises(ValueError):
            member_seed(0, *bad)


def test_dropout_seed_nests_restores_and_leaves_the_counter_alone():
    import tecmollm
    from src.model import modules as M_
    from tecmollm import functions as F_
    assert tecmollm.dropout_seed is F_.dropout_seed is M_.dropout_seed
    mod = torch.nn.Linear(1, 1)
    torch.manual_seed(99)
    M_._seed_counter[0] = 4
    assert M_.make_plan(mod).base_seed == 99 + 7919 * 5                    # as before this context existed
    with tecmollm.dropout_seed(1234):
        assert M_.make_plan(mod).base_seed == 1234 and M_.make_plan(mod).base_seed == 1234
        with tecmollm.dropout_seed(77):
            assert M_.make_plan(mod).base_seed == 77
        assert M_.make_plan(mod).base_seed == 1234
        with pytest.raises(RuntimeError):
            with tecmollm.dropout_seed(5):
                raise RuntimeError("a forward that raises")
        assert M_.make_plan(mod).base_seed == 1234
    assert F_.pinned_dropout_seed() is None
    assert M_._seed_counter[0] == 10                                       # five plans inside: the counter moved on
    assert M_.make_plan(mod).base_seed == 99 + 7919 * 11
    plan = M_.make_plan(mod.train())
    assert plan.training and plan.spec(F_.SITE_HEAD, 8) is not None


def _descriptor(**over):
    from tecmollm import _lib
    buf = (ctypes.c_double * 8)()                                          # a real, aligned host address: never dereferenced
    a = ctypes.addressof(buf)
    fields = dict(members=a, m_stride_k=1, m_stride_s=1, m_stride_h=1, m_stride_i=1, target=a, t_stride_s=1, t_stride_h=1,
                  t_stride_i=1, S=1, H=1, G=1, I=1, K=8, trim=1, mean=0.0, scale=1.0, clip_lo=0.0, clip_hi=200.0, clip=0,
                  stats=a, hist=a, group=None, err_flag=a)
    fields.update(over)
    e = _lib.TecmEnsemble(**fields)
    e._keep = buf
    return e


@pytest.mark.parametrize("over, text", [
    (dict(K=1), b"outside [2, 64]"), (dict(K=0), b"outside [2, 64]"), (dict(K=65), b"outside [2, 64]"),
    (dict(K=8, trim=4), b"2 * trim < K - 1"), (dict(K=2, trim=1), b"2 * trim < K - 1"), (dict(trim=-1), b"2 * trim < K - 1"),
    (dict(K=3, trim=1), b"2 * trim < K - 1"),
    (dict(scale=0.0), b"scale must be non-zero"),
    (dict(members=None), b"null pointer"), (dict(target=None), b"null pointer"), (dict(stats=None), b"null pointer"),
    (dict(hist=None), b"null pointer"), (dict(err_flag=None), b"null pointer"),
    (dict(S=0), b"bad shape"), (dict(H=0), b"bad shape"), (dict(I=0), b"bad shape"), (dict(G=0), b"bad shape"),
    (dict(G=65536), b"<= 65535"), (dict(I=1 << 40), b"2^24 blocks"),
])
def test_the_launcher_rejects_bad_descriptors_before_any_device_call(over, text):
    from tecmollm import _lib
    e = _descriptor(**over)
    rc = _lib.lib().tecm_ensemble_stats(ctypes.byref(e), None)
    assert rc == -1, (over, rc)                                            # TECM_E_ARG
    assert text in _lib.lib().tecm_last_error(), (over, _lib.lib().tecm_last_error())


def test_the_launcher_rejects_misaligned_pointers_and_a_null_descriptor():
    from tecmollm import _lib
    assert _lib.lib().tecm_ensemble_stats(None, None) == -1
    assert b"null descriptor" in _lib.lib().tecm_last_error()
    e = _descriptor()
    e.stats += 4
    assert _lib.lib().tecm_ensemble_stats(ctypes.byref(e), None) not in (0, -1)       # TECM_E_ALIGN
    assert b"8-byte aligned" in _lib.lib().tecm_last_error()


def test_header_binding_and_wrappers_agree_on_the_new_symbols():
    from src.evaluation import metrics as M
    from tecmollm import _lib, ops
    header = open(os.path.join(ROOT, "include", "tecmollm.h")).read()
    assert "#define TECM_ENS_STATS 9" in header and _lib.TECM_ENS_STATS == 9 == ER.STATS
    assert "#define TECM_ENS_MAX_K 64" in header and _lib.TECM_ENS_MAX_K == 64
    assert "int tecm_ensemble_stats(const TecmEnsemble* e, void* stream);" in header
    assert "tecm_ensemble_stats" in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "tecm_ensemble_stats")
    assert _lib.ABI_VERSION == 21 and _lib.lib().tecm_abi_version() == 21     # an additive entry point: the version stays
    # the struct: the same field names in the same order as the header's
    body = re.search(r"typedef struct \{([^}]*)\} TecmEnsemble;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"[\s*](\w+)\s*[,;]", body)
    assert names == [f[0] for f in _lib.TecmEnsemble._fields_]
    assert ctypes.sizeof(_lib.TecmEnsemble) == 8 * 9 + 8 + 4 + 4 + 8 + 4 + 4 + 16 + 16 + 8 * 4 + 8 * 5 + 8 * 3
    assert callable(ops.ensemble_stats) and ops.ENSEMBLE_OUTPUTS == ("mean", "std", "lo", "hi", "mean_raw")
    assert len(M.ENSEMBLE_KEYS) == 10


def _prob(G=2, H=3, I=6, K=4, trim=1):
    from src.evaluation.metrics import EnsembleMetrics
    rng = np.random.default_rng(8)
    m = rng.standard_normal((K, 9, H, I)).astype(np.float32)
    t = rng.standard_normal((9, H, I)).astype(np.float32)
    stats, mags, hist = np.zeros((G, H, 9, I)), np.zeros((G, H, 9, I)), np.zeros((G, H, K + 1, I), dtype=np.int64)
    ER.accumulate(stats, mags, hist, m, t, None, None, trim)              # group 1 is never visited
    em = EnsembleMetrics(H, I, K, G, None, trim, device="cpu")
    em.stats.copy_(torch.from_numpy(stats))
    em.hist.copy_(torch.from_numpy(hist).to(torch.int32))
    return em.compute()


@pytest.mark.parametrize("grid", [None, (2, 3)])
def test_write_ensemble_round_trips(tmp_path, grid):
    from src.evaluation.metrics import ENSEMBLE_KEYS
    from tecmollm import write_ensemble
    from tecmollm.ensemble import CSV_COLUMNS
    prob = _prob()
    paths = write_ensemble(prob, str(tmp_path / "out"), grid=grid)
    assert sorted(os.listdir(tmp_path / "out")) == ["ensemble_by_horizon.csv", "ensemble_maps.npz"]
    z = np.load(paths["npz"])
    assert sorted(z.files) == sorted(ENSEMBLE_KEYS + ("rank_histogram", "nominal_coverage"))
    for k in ENSEMBLE_KEYS:
        assert z[k].shape == ((2, 3, 6) if grid is None else (2, 3, 2, 3))
        assert np.array_equal(z[k].reshape(2, 3, 6), prob[k], equal_nan=True)
    assert np.array_equal(z["rank_histogram"], prob["rank_histogram"]) and float(z["nominal_coverage"]) == 1 / 5
    with open(paths["csv"], newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["group", "horizon"] + list(CSV_COLUMNS)
    assert CSV_COLUMNS == ("crps", "fair_crps", "rmse_mean", "spread", "spread_skill", "coverage", "nominal_coverage",
                           "interval_width")
    assert [(r[0], r[1]) for r in rows[1:]] == [(str(g), str(h)) for g in range(2) for h in range(3)]
    for r in rows[1:]:
        pooled = prob["by_group"][int(r[0])]
        for cell, k in zip(r[2:], CSV_COLUMNS):
            want = prob["nominal_coverage"] if k == "nominal_coverage" else pooled[f"{k}_by_horizon"][int(r[1])]
            assert float(cell) == want or (np.isnan(float(cell)) and np.isnan(want)), (r, k)
    with pytest.raises(ValueError):
        write_ensemble(prob, str(tmp_path / "bad"), grid=(4, 2))
