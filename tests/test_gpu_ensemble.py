"""GPU tests of the ensemble scores: the kernel (tecm_ensemble_stats) through `EnsembleMetrics` against the float64 numpy
restatement that adds in the kernel's order (tests/ensemble_ref.py), its per-sample outputs, its determinism, its group-id
check; the seeded stochastic forward (`dropout_seed`, `ensemble_members`) on a tiny model, bit for bit and against the CPU
oracle with the same masks; `evaluate_ensemble` / `ensemble_forecast` / `write_ensemble` end to end.

The bar of every comparison with the restatement is the error maps' (tests/test_gpu_error_maps.py) and for the same reason:
per statistic |kernel - numpy| <= 1e-12 * sum |terms|, the sum taken from the restatement.  Both sides add the same terms
in the same order in float64, so only FMA contraction inside a term (d*d, c*x) and a few dozen roundings lie between them;
counts and rank histograms are integers and must match exactly."""
import os

import numpy as np
import pytest
import torch

from tests import ensemble_ref as ER

pytestmark = pytest.mark.gpu

BAR = 1e-12
SCALER = (21.5, 9.25)
BASE = dict(K=8, S=5, H=12, I=65, G=3, trim=1, scaler=True, members="contiguous", target="dataset")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _values(K, S, H, I, rng, scaler):
    """Scaled members (K, S, H, I) and truths (S, H, I) with everything hard in them: NaN and both infinities in both,
    members tied at both clip bounds (far outside [0, 200] TECU once unscaled), truths copied from a member."""
    m = (rng.standard_normal((K, S, H, I)) * 2.5).astype(np.float32)
    t = (rng.standard_normal((S, H, I)) * 2.5).astype(np.float32)
    m[rng.random(m.shape) < 0.2] = np.float32(-30.0)
    m[rng.random(m.shape) < 0.1] = np.float32(+40.0)
    copy = rng.random(t.shape) < 0.25
    t[copy] = m[rng.integers(K)][copy]
    for a in (m.reshape(-1), t.reshape(-1)):
        if a.size >= 6:
            w = rng.choice(a.size, size=3, replace=False)
            a[w[0]], a[w[1]], a[w[2]] = np.nan, np.inf, -np.inf
    return m, t


def _on_device(m, t, members, target, dev):
    """Device views holding m (K, S, H, I) and t (S, H, I) with the strides the layout names say."""
    md = torch.from_numpy(m).to(dev)
    if members == "permuted":                      # stored (S, I, K, H): stride_h = 1, stride_k = H, stride_i = K*H
        md = md.permute(1, 3, 0, 2).contiguous().permute(2, 0, 3, 1)
        assert md.stride(2) == 1 and md.stride(3) != 1
    else:
        assert md.stride(3) == 1 or md.shape[3] == 1
    td = torch.from_numpy(t).to(dev)
    if target == "model":                          # the model's output layout: (S, I, H) permuted, stride_h = 1, stride_i = H
        td = td.permute(0, 2, 1).contiguous().permute(0, 2, 1).unsqueeze(-1)
    else:                                          # the dataset's (S, H, N, 1)
        td = td.unsqueeze(-1)
    return md, td


def _assert_close(got, want, mags, what):
    err = np.abs(got - want)
    worst = float(np.max(err / np.maximum(mags, 1e-300)))
    print(f"{what}: max |kernel - numpy| / sum|terms| = {worst:.3e}")
    assert np.all(err <= BAR * mags), (what, worst)


def _ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def _check_outputs(outs, q, keep, what):
    """Per-sample outputs of one update against the restatement `q`, on the samples `keep` (a bool mask over s)."""
    got = {k: v.cpu().numpy()[keep] for k, v in outs.items()}
    assert np.array_equal(got["lo"], q["lo"][keep]) and np.array_equal(got["hi"], q["hi"][keep]), what
    mr = q["mean_raw"][keep]
    want = mr.astype(np.float32)
    # the float32 rounding of the float64 mean is unambiguous unless a neighbouring float64 rounds the other way
    sure = (np.nextafter(mr, np.inf).astype(np.float32) == want) & (np.nextafter(mr, -np.inf).astype(np.float32) == want)
    # (the mean of K floats is often an exact float32 tie -- one bit more than 24 for K = 2 -- and counts as ambiguous here,
    #  up to about every second value; the 1-ulp comparison below covers those)
    assert sure.mean() > 0.25
    assert np.array_equal(got["mean_raw"][sure], want[sure]), what
    assert np.all(np.abs(got["mean_raw"].astype(np.float64) - want) <= _ulp32(want)), what
    for k, ref in (("mean", q["mu"][keep]), ("std", np.sqrt(q["var"][keep]))):
        r32 = ref.astype(np.float32)
        assert np.all(np.abs(got[k].astype(np.float64) - r32) <= _ulp32(r32)), (what, k)


def _cases():
    out = [dict(BASE)]
    for key, vals in (("K", (2, 3, 17, 33, 64)), ("I", (1, 63, 64, 135)), ("H", (1, 33)), ("S", (1, 17)), ("G", (1,)),
                      ("scaler", (False,)), ("members", ("permuted",)), ("target", ("model",))):
        out += [dict(BASE, **{key: v}) for v in vals]
    out += [dict(BASE, trim=0), dict(BASE, trim=3), dict(BASE, K=64, trim=31),
            dict(BASE, K=17, trim=7, members="permuted", target="model")]
    for c in out:                                   # trim must stay legal where K shrinks
        if not 2 * c["trim"] < c["K"] - 1:
            c["trim"] = 0
    return out


@pytest.mark.parametrize("case", _cases(), ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items() if BASE[k] != v) or "base")
def test_statistics_match_the_ordered_float64_restatement(dev, case):
    """One axis at a time around K = 8, S = 5, H = 12, I = 65, G = 3: K at the minimum, on both sides of the padded sizes and
    at the maximum; I over the tile edge; H, S; one group and three (ids out of order, group 1 never visited and pre-filled
    with a sentinel that must survive); trim 0, 1 and the largest legal; with and without scaler + clip; both member and
    both target layouts.  Every case: two consecutive updates into one object, hard values in both operands, the
    per-sample outputs on the first update and null output pointers on the second."""
    from src.evaluation.metrics import EnsembleMetrics
    from tecmollm import check_device_errors, ops
    K, S, H, I, G, trim = (case[k] for k in ("K", "S", "H", "I", "G", "trim"))
    scaler = SCALER if case["scaler"] else None
    rng = np.random.default_rng(sum(map(ord, repr(sorted(case.items())))))
    em = EnsembleMetrics(H, I, K, G, scaler, trim, device=dev)
    want, mags = np.zeros((G, H, 9, I)), np.zeros((G, H, 9, I))
    hist = np.zeros((G, H, K + 1, I), dtype=np.int64)
    if G == 3:
        em.stats[1].copy_(torch.arange(H * 9 * I, device=dev, dtype=torch.float64).view(H, 9, I) + 0.5)
        em.hist[1].copy_(torch.arange(H * (K + 1) * I, device=dev, dtype=torch.int32).view(H, K + 1, I) + 7)
        sentinel = em.stats[1].clone(), em.hist[1].clone()
    for update in range(2):
        m, t = _values(K, S, H, I, rng, scaler)
        md, td = _on_device(m, t, case["members"], case["target"], dev)
        ids = None
        if G == 3:
            ids = np.resize(np.array([2, 0, 2, 0, 2] if update == 0 else [0, 2, 2, 0, 0], dtype=np.int32), S)
        elif update == 1:
            ids = np.zeros(S, dtype=np.int32)                                  # the same as None
        outs = em.update(md, td, None if ids is None else torch.from_numpy(ids).to(dev),
                         outputs=ops.ENSEMBLE_OUTPUTS if update == 0 else ())
        q = ER.accumulate(want, mags, hist, m, t, ids, scaler, trim)
        if update == 0:
            assert set(outs) == set(ops.ENSEMBLE_OUTPUTS)
            _check_outputs(outs, q, np.ones(S, dtype=bool), repr(case))
        else:
            assert outs == {}
    got, got_hist = em.stats.cpu().numpy(), em.hist.cpu().numpy().astype(np.int64)
    if G == 3:
        assert torch.equal(em.stats[1], sentinel[0]) and torch.equal(em.hist[1], sentinel[1]), "the never-visited group was touched"
        got[1] = want[1] = 0
        got_hist[1] = hist[1] = 0
    _assert_close(got, want, mags, repr(case))
    assert np.array_equal(got[:, :, 0], want[:, :, 0]) and got[:, :, 0].sum() == 2 * S * H * I      # the counts, exactly
    assert np.array_equal(got_hist, hist)
    assert np.array_equal(got_hist.sum(axis=2), want[:, :, 0].astype(np.int64))                    # every sample has one rank
    check_device_errors()                                                                          # no id was out of range


def test_three_accumulations_at_full_size_hold_identical_bits(dev):
    """N = 2911, H = 12, B = 16, K = 16, four groups, two batches: one owner per cell and no atomics, so three fresh
    accumulations agree bit for bit, in the statistics and in the histograms."""
    from src.evaluation.metrics import EnsembleMetrics
    gen = torch.Generator(device=dev).manual_seed(5)
    batches = []
    for b in range(2):
        m = torch.randn(16, 16, 12, 2911, device=dev, generator=gen) * 1.5
        t = torch.randn(16, 12, 2911, 1, device=dev, generator=gen) * 1.5
        ids = torch.from_numpy(((np.arange(16) * 7 + b) % 4).astype(np.int32)).to(dev)
        batches.append((m, t, ids))
    runs = []
    for _ in range(3):
        em = EnsembleMetrics(12, 2911, 16, 4, SCALER, 1, device=dev)
        for m, t, ids in batches:
            em.update(m, t, ids)
        runs.append((em.stats.clone(), em.hist.clone()))
    for st, hs in runs[1:]:
        assert torch.equal(st, runs[0][0]) and torch.equal(hs, runs[0][1])
    assert float(runs[0][0][:, :, 0].sum()) == 32 * 12 * 2911 == int(runs[0][1].sum())
    out = em.compute()
    assert out["crps"].shape == (4, 12, 2911) and np.isfinite(out["crps"]).all() and (out["crps"] >= 0).all()


def test_a_group_id_out_of_range_is_skipped_and_reported(dev):
    """One sample with id = G (and, in a second object, one with id -1): the other samples are accumulated, no cell and no
    histogram takes the bad sample, its per-sample outputs are not written, and check_device_errors() raises TecmError
    naming TECM_BAD_GROUP once.  An error flag, not a fault."""
    from src.evaluation.metrics import EnsembleMetrics
    from tecmollm import TecmError, check_device_errors
    check_device_errors()
    rng = np.random.default_rng(12)
    for bad in (3, -1):
        K, S, H, I, G = 8, 5, 12, 65, 3
        m, t = _values(K, S, H, I, rng, SCALER)
        md, td = _on_device(m, t, "contiguous", "dataset", dev)
        ids = np.array([0, bad, 1, 2, 0], dtype=np.int32)
        em = EnsembleMetrics(H, I, K, G, SCALER, 1, device=dev)
        outs = em.update(md, td, torch.from_numpy(ids).to(dev), outputs=("lo", "hi", "mean", "std", "mean_raw"))
        want, mags, hist = np.zeros((G, H, 9, I)), np.zeros((G, H, 9, I)), np.zeros((G, H, K + 1, I), dtype=np.int64)
        q = ER.accumulate(want, mags, hist, m, t, ids, SCALER, 1)          # skips the sample, as the kernel must
        got = em.stats.cpu().numpy()
        _assert_close(got, want, mags, f"bad id {bad}")
        assert got[:, :, 0].sum() == 4 * H * I == int(em.hist.sum())       # four samples counted, nowhere a fifth
        assert np.array_equal(em.hist.cpu().numpy(), hist)
        _check_outputs(outs, q, ids != bad, f"bad id {bad}")
        with pytest.raises(TecmError, match="TECM_BAD_GROUP"):
            check_device_errors()
        check_device_errors()                                              # reported once, then clear


# ------------------------------------------------------------------------------------ the seeded stochastic forward
CFG_KW = dict(L_in=16, L_out=12, num_nodes=12)


@pytest.fixture(scope="module")
def tiny(dev):
    from oracle import ref_cpu as R
    from tests.parity import build_model
    cfg = R.default_config(**CFG_KW)
    params = R.init_params(cfg, seed=3)
    model = build_model(cfg, params, dev, "per_timestep").eval()
    B = 2
    x, tf, _ = R.synthetic_batch(B, cfg["temporal_seq_len"], 12, cfg["spatial_in_channels_base"], cfg["prediction_horizon"],
                                 seed=103)
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0]
    tfd = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(B, cfg["temporal_seq_len"], 12, 4)
    return dict(cfg=cfg, params=params, model=model, x=x, tf=tf, ei=ei, xd=x.to(dev), tfd=tfd, eid=ei.to(dev), B=B)


def test_ensemble_members_are_reproducible_and_are_plain_seeded_forwards(dev, tiny):
    from tecmollm import dropout_seed, ensemble_members, member_seed
    model, xd, tfd, eid = tiny["model"], tiny["xd"], tiny["tfd"], tiny["eid"]
    for start in (False, True):
        model.train(start)
        a = ensemble_members(model, xd, tfd, eid, 4, seed=11, chunk=2)
        assert model.training is start                                     # restored, for both initial states
    assert a.shape == (4, tiny["B"], 12, 12) and a.dtype == torch.float32 and a.is_contiguous() and a.is_cuda
    assert model.recompute_level == 0                                      # no grad: the lean forward, nothing recomputed
    model.eval()
    b = ensemble_members(model, xd, tfd, eid, 4, seed=11, chunk=2)
    c = ensemble_members(model, xd, tfd, eid, 4, seed=12, chunk=2)
    d = ensemble_members(model, xd, tfd, eid, 4, seed=11, chunk=3)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, d)
    assert len({a[k].cpu().numpy().tobytes() for k in range(4)}) == 4      # four different members
    with torch.no_grad():
        plain = model(xd, tfd, eid).squeeze(-1)                            # eval: no dropout
        assert not torch.equal(plain, a[0])
        model.train()
        try:
            for k in range(4):
                with dropout_seed(member_seed(11, 2, k)):
                    y = model(xd, tfd, eid)
                assert torch.equal(y.squeeze(-1), a[k]), k                 # bit for bit
        finally:
            model.eval()

    class Boom(RuntimeError):
        pass

    def boom(*args, **kw):
        raise Boom()
    handle = model.register_forward_pre_hook(boom)
    try:
        with pytest.raises(Boom):
            ensemble_members(model, xd, tfd, eid, 2, seed=1)
    finally:
        handle.remove()
    assert model.training is False                                         # restored when a forward raises, too
    with pytest.raises(ValueError):
        ensemble_members(model, xd, tfd, eid, 0, seed=0)
    with pytest.raises(ValueError):
        ensemble_members([], xd, tfd, eid, 2, seed=0)
    twice = ensemble_members([model, model], xd, tfd, eid, 3, seed=0)      # a sequence of models: one member each, 3 ignored
    assert twice.shape[0] == 2 and torch.equal(twice[0], plain) and torch.equal(twice[1], plain)


def test_one_member_matches_the_cpu_oracle_fed_the_same_masks(dev, tiny):
    """Member 1 of (seed 11, chunk 2) against oracle.ref_cpu.forward with `device_masks` of that member's base seed, at the
    bars of every train-mode forward here (tests/parity.assert_close: 1e-3 max-norm and element-wise)."""
    from oracle import ref_cpu as R
    from tecmollm import ensemble_members, member_seed
    from tests.parity import assert_close, device_masks
    cfg = tiny["cfg"]
    mem = ensemble_members(tiny["model"], tiny["xd"], tiny["tfd"], tiny["eid"], 2, seed=11, chunk=2)
    masks = device_masks(cfg, tiny["B"], tiny["ei"], member_seed(11, 2, 1), "per_timestep")
    with torch.no_grad():
        ref = R.forward(tiny["x"], tiny["tf"], tiny["ei"], tiny["params"], cfg, None, masks=masks)
    assert_close(mem[1].unsqueeze(-1), ref, "member 1 vs oracle")
    with torch.no_grad():
        ref0 = R.forward(tiny["x"], tiny["tf"], tiny["ei"], tiny["params"], cfg, None)
    assert float((ref - ref0).abs().max()) > 1e-2 * float(ref0.abs().max())    # the masks matter at this bar


# ------------------------------------------------------------------------------------ evaluate_ensemble end to end
KEYS = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg", "mae_by_horizon", "rmse_by_horizon", "r2_by_horizon",
        "pearson_by_horizon")


@pytest.fixture(scope="module")
def split(dev, golden_dir, tiny):
    from src.data.dataset import SlidingWindowSamplerDataset
    g = np.load(os.path.join(golden_dir, "evaluate_split.npz"))
    X = torch.as_tensor(g["X"])
    ds = SlidingWindowSamplerDataset.from_tensors(X, torch.as_tensor(g["Y"]), torch.as_tensor(g["TF"]), int(g["L_in"]),
                                                  int(g["L_out"]), stride=1, device=dev, mode="test")
    return g, tiny["model"], ds, tiny["eid"], (float(g["mean"]), float(g["scale"]))


def test_evaluate_ensemble_end_to_end_on_a_tiny_model(dev, split, tiny, tmp_path):
    """12 nodes, 24 windows, batch size 5 (a ragged last batch), K = 4."""
    from oracle import ref_cpu as R
    from src.evaluation.metrics import ENSEMBLE_KEYS, EnsembleMetrics, HorizonMetrics
    from tecmollm import ensemble as EN
    from tecmollm import evaluate as E
    from tests.parity import build_model
    g, model, ds, ei, scaler = split
    S, N, H, K = len(ds), 12, 12, 4
    assert S % 5 != 0
    want = E.evaluate_split(model, ds, ei, 5, scaler=scaler, baselines=("mean", "last"))
    slots = E.window_groups_by_slot(ds)
    res, maps, prob = EN.evaluate_ensemble(model, ds, ei, 5, members=K, seed=3, scaler=scaler, trim=1,
                                           baselines=("mean", "last"), groups=slots, num_groups=12)
    assert model.training is False
    assert list(res) == list(maps) == ["TEC-MoLLM", "HistoricalAverage", "Persistence", "TEC-MoLLM-MC"]
    for name in want:
        assert set(res[name]) == set(want[name]) == set(KEYS)
        for k in KEYS:
            assert res[name][k] == want[name][k], (name, k)                # exactly
    # the MC entry: a HorizonMetrics fed the mean of the members computed on the host (float64 mean over k ascending)
    hm = HorizonMetrics(H, scaler, device=dev)
    host_counts = np.zeros(12, dtype=np.int64)
    mags = np.zeros((H, 8))
    from tests.error_maps_ref import pipeline, terms
    for ordinal, chunk in enumerate([list(range(a, min(a + 5, S))) for a in range(0, S, 5)]):
        x, tf, y = ds.batch(chunk)
        mem = EN.ensemble_members(model, x, tf, ei, K, 3, ordinal)
        mean = mem.double().cpu().numpy()
        acc = np.zeros(mean.shape[1:])
        for k in range(K):
            acc = acc + mean[k]
        mean32 = (acc / K).astype(np.float32)
        hm.update(torch.from_numpy(mean32).to(dev).unsqueeze(-1), y)
        t, p = pipeline(mean32, y.squeeze(-1).cpu().numpy(), scaler)
        mags += np.abs(terms(t, p)).sum(axis=(1, 3)).T
    # the `collapse` bar of the error-map tests: |a - b| <= 1e-12 * sum |terms| on the (H, 8) statistics (the two sides
    # add the same (t, p) pairs, HorizonMetrics with atomics in no fixed order); the numbers derived from them to 1e-9
    kept = []
    orig = HorizonMetrics.compute

    def spy(self):
        kept.append(self.stats.clone())
        return orig(self)
    HorizonMetrics.compute = spy
    try:
        res2, maps2, prob2 = EN.evaluate_ensemble(model, ds, ei, 5, members=K, seed=3, scaler=scaler, trim=1,
                                                  baselines=("mean", "last"), groups=slots, num_groups=12)
    finally:
        HorizonMetrics.compute = orig
    assert len(kept) == 4                                                  # the fourth forecast is the MC mean
    err = np.abs(kept[3].cpu().numpy() - hm.stats.cpu().numpy())
    print("MC collapse: max err / sum|terms| =", float((err / np.maximum(mags, 1e-300)).max()))
    assert np.all(err <= BAR * mags)
    mc = hm.compute()
    for k in KEYS:
        np.testing.assert_allclose(np.asarray(res["TEC-MoLLM-MC"][k]), np.asarray(mc[k]), rtol=1e-9, atol=1e-12, err_msg=k)
    for k in ENSEMBLE_KEYS:                                                # the same seed: the same scores, bit for bit
        assert np.array_equal(prob[k], prob2[k], equal_nan=True), k
    # counts, histograms, coverage
    assert set(prob) == set(ENSEMBLE_KEYS) | {"nominal_coverage", "rank_histogram", "by_group"}
    assert prob["nominal_coverage"] == (K - 2 - 1) / (K + 1)
    host = slots.tolist()
    assert prob["count"].shape == (12, H, N) and prob["count"].sum() == S * H * N
    rh = prob["rank_histogram"]
    assert rh.shape == (12, H, K + 1)
    for s in range(12):
        assert (prob["count"][s] == host.count(s)).all()
        assert (rh[s].sum(axis=1) == host.count(s) * N).all()              # each group's histogram sums to its count
        if host.count(s) == 0:
            assert np.isnan(prob["crps"][s]).all() and np.isnan(prob["by_group"][s]["crps_avg"])
        else:
            pooled = prob["by_group"][s]
            np.testing.assert_allclose(pooled["coverage_by_horizon"], rh[s][:, 2:K - 1].sum(axis=1) / (host.count(s) * N),
                                       rtol=1e-15)
            assert np.isfinite(prob["crps"][s]).all() and (prob["fair_crps"][s] <= prob["crps"][s] + 1e-12).all()
    # two shards cut at a batch boundary (what two ranks would score), the second numbering its batches after the first's
    # three: the same members as in the single pass, statistics and histograms added by hand
    kept_em = []
    orig_em = EnsembleMetrics.compute

    def spy_em(self):
        kept_em.append((self.stats.clone(), self.hist.clone()))
        return orig_em(self)
    EnsembleMetrics.compute = spy_em
    try:
        for order, first in ((list(range(15)), 0), (list(range(15, S)), 3)):
            EN.evaluate_ensemble(model, ds, ei, 5, members=K, seed=3, scaler=scaler, trim=1, groups=slots, num_groups=12,
                                 order=order, first_chunk=first)
    finally:
        EnsembleMetrics.compute = orig_em
    merged = EnsembleMetrics(H, N, K, 12, scaler, 1, device=dev)
    merged.stats.copy_(kept_em[0][0] + kept_em[1][0])
    merged.hist.copy_(kept_em[0][1] + kept_em[1][1])
    out = merged.compute()
    for k in ENSEMBLE_KEYS:
        np.testing.assert_allclose(out[k], prob[k], rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=k)
    assert np.array_equal(out["rank_histogram"], prob["rank_histogram"])
    # a deep ensemble: two differently initialised models, one eval-mode member each
    cfg = tiny["cfg"]
    other = build_model(cfg, R.init_params(cfg, seed=4), dev, "per_timestep").train()
    resd, mapsd, probd = EN.evaluate_ensemble([model, other], ds, ei, 5, scaler=scaler, trim=0)     # members: not used
    assert other.training is True and model.training is False
    assert probd["count"].shape == (1, H, N) and probd["count"].sum() == S * H * N and probd["nominal_coverage"] == 1 / 3
    for k in KEYS:
        assert resd["TEC-MoLLM"][k] == want["TEC-MoLLM"][k]
    x, tf, y = ds.batch([0, 1])
    two = EN.ensemble_members([model, other], x, tf, ei, None, seed=0)
    with torch.no_grad():
        other.eval()
        assert torch.equal(two[0], model(x, tf, ei).squeeze(-1)) and torch.equal(two[1], other(x, tf, ei).squeeze(-1))
    assert float((two[0] - two[1]).abs().max()) > 0
    # the forecast with its error bar
    fc = EN.ensemble_forecast(model, x, tf, ei, members=K, seed=3, scaler=scaler, trim=1)
    assert set(fc) == {"mean", "std", "lo", "hi", "members", "nominal_coverage"} and fc["nominal_coverage"] == 1 / 5
    assert fc["members"].shape == (K, 2, H, N) and all(fc[k].shape == (2, H, N) and fc[k].is_cuda for k in ("mean", "std", "lo", "hi"))
    x_phys = ER.values(fc["members"].cpu().numpy(), np.zeros((2, H, N), dtype=np.float32), scaler)[0]
    srt = np.sort(x_phys, axis=0)
    assert np.array_equal(fc["lo"].cpu().numpy(), srt[1]) and np.array_equal(fc["hi"].cpu().numpy(), srt[K - 2])
    np.testing.assert_allclose(fc["mean"].cpu().numpy(), x_phys.astype(np.float64).mean(axis=0), rtol=3e-7)
    np.testing.assert_allclose(fc["std"].cpu().numpy(), x_phys.astype(np.float64).std(axis=0, ddof=1), rtol=1e-5, atol=1e-6)
    assert (fc["lo"] <= fc["hi"]).all() and (fc["std"] > 0).any()
    # the files
    paths = EN.write_ensemble(prob, str(tmp_path / "out"), grid=(3, 4))
    z = np.load(paths["npz"])
    assert sorted(z.files) == sorted(ENSEMBLE_KEYS + ("rank_histogram", "nominal_coverage"))
    assert z["crps"].shape == (12, H, 3, 4) and z["rank_histogram"].shape == (12, H, K + 1)
    with open(paths["csv"], encoding="utf-8") as f:
        lines = f.read().splitlines()
    assert lines[0] == "group,horizon," + ",".join(EN.CSV_COLUMNS) and len(lines) == 1 + 12 * H
