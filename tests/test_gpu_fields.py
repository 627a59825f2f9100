"""GPU tests of the field scores: the kernels (tecm_field_scores) through `FieldMetrics` against the float64 numpy
restatement (tests/fields_ref.py), their determinism, their group-id check; the shuffled-against-coherent ensembles on the
device; `evaluate_ensemble(..., fields=)`, `evaluate_analog_ensemble(..., fields=)` and `write_fields` end to end.

The bars (none of them comes from what the kernels give):
  counts       the sample counts and the pair counts are integers and must match exactly;
  energy sums  |kernel - numpy| <= (I + K^2 + S + 16) * 2^-53 * (sum of the norms that enter), S the samples that entered:
               both sides work in float64 and every term is non-negative, so the bound holds for any order of the additions;
  variogram    per (g, h, class), with delta = (K + 4) * 2^-23 * (v_o + v_e) per pair from the restatement (the kernel's
               per-pair term is float32: difference, square root, k-ascending sum, one division -- K + 4 roundings at most):
               |kernel - numpy| <= sum (2 |e| + delta) delta for sum e^2, sum (2 + delta) delta for sum v_o and sum v_e.
               About 1e-5 of the value: one lost pair fails it."""
import os

import numpy as np
import pytest
import torch

from tests import fields_ref as FR
from tests.test_gpu_ensemble import _on_device, _values

pytestmark = pytest.mark.gpu

SCALER = (21.5, 9.25)
BASE = dict(K=8, S=5, H=12, I="T+1", G=3, NB=4, order=0.5, scaler=True, members="contiguous", target="dataset", classes="random")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _classes(I, NB, kind, rng):
    """(I, I) uint8: above the diagonal classes drawn from [0, NB) and 255, with the class NB - 2 never drawn where NB >= 3
    ("random"), or nothing but excluded pairs ("excluded"); the diagonal and the lower triangle hold VALID class numbers,
    which the kernel must never read."""
    if NB == 0:
        return None
    pool = [c for c in range(NB) if not (NB >= 3 and c == NB - 2)] + [255, NB] if kind == "random" else [255, NB, 200]
    pc = rng.choice(np.array(pool, dtype=np.uint8), size=(I, I))
    low = np.tril_indices(I)
    pc[low] = rng.integers(0, NB, size=low[0].size).astype(np.uint8)
    return pc


def _nodes(spec, T):
    return {"1": 1, "2": 2, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}[spec]


def _cases():
    out = [dict(BASE)]
    for key, vals in (("I", ("1", "2", "T-1", "T", "2T+3")), ("K", (1, 2)), ("H", (1,)), ("NB", (0, 1, 16)),
                      ("order", (1.0, 2.0)), ("scaler", (False,)), ("members", ("permuted",)), ("target", ("model",)),
                      ("classes", ("excluded",))):
        out += [dict(BASE, **{key: v}) for v in vals]
    out += [dict(BASE, K=64, H=1), dict(BASE, K=64, H=1, NB=16, I="2T+3"),           # the smaller tile: K and NB at their limits
            dict(BASE, K=2, I="2T+3", members="permuted", target="model", order=2.0, scaler=False)]
    return out


def _check(got_es, got_vs, want_es, mags, want_vs, bound, I, K, S, what):
    assert np.array_equal(got_es[..., 0], want_es[..., 0]), what                         # sample counts
    assert np.array_equal(got_vs[..., :2], want_vs[..., :2]), what                       # sample counts, pair counts
    bar = FR.energy_bar(I, K, S, mags[..., 1:])
    err = np.abs(got_es[..., 1:] - want_es[..., 1:])
    print(f"{what}: energy max err / bar = {float(np.max(err / np.maximum(bar, 1e-300))):.3e}")
    assert np.all(err <= bar), what
    if want_vs.shape[-2]:
        verr = np.abs(got_vs[..., 2:] - want_vs[..., 2:])
        print(f"{what}: variogram max err / bar = {float(np.max(verr / np.maximum(bound, 1e-300))):.3e}; "
              f"bar / value = {float(np.max(bound[..., 0] / np.maximum(want_vs[..., 2], 1e-300))):.3e}")
        assert np.all(verr <= bound), what


@pytest.mark.parametrize("case", _cases(), ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items() if BASE[k] != v) or "base")
def test_sums_match_the_float64_restatement(dev, case):
    """One axis at a time around K = 8, S = 5, H = 12, I = T + 1, G = 3, NB = 4, order 0.5 (T from the library's plan): I below,
    at and above one tile and over two; K = 1, 2, 64; H = 1; NB = 0, 1, 16, a class that stays empty and a matrix that excludes
    every pair; the three orders; with and without scaler + clip; both member and both target layouts.  Every case: two
    updates into one object (ids out of order, group 1 never visited and pre-filled with a sentinel that must survive),
    hard values in both operands (NaN, both infinities, members tied at the clip bounds), the per-sample outputs on the
    first update, and a second object fed the same updates, which must hold the same bits."""
    from src.evaluation.metrics import FieldMetrics
    from tecmollm import check_device_errors, ops
    K, S, H, G, NB, order = (case[k] for k in ("K", "S", "H", "G", "NB", "order"))
    T = ops.field_scores_plan(S, H, 1000, K, NB)[0]
    I = _nodes(case["I"], T)
    scaler = SCALER if case["scaler"] else None
    rng = np.random.default_rng(sum(map(ord, repr(sorted(case.items())))))
    pc = _classes(I, NB, case["classes"], rng)
    pcd = None if pc is None else torch.from_numpy(pc).to(dev)
    fms = [FieldMetrics(H, I, K, pcd, NB, order, G, scaler, device=dev) for _ in range(2)]
    want_es, mags = np.zeros((G, H, 4)), np.zeros((G, H, 4))
    want_vs, bound = np.zeros((G, H, NB, 5)), np.zeros((G, H, NB, 3))
    for fm in fms:
        fm.es_stats[1].copy_(torch.arange(H * 4, device=dev, dtype=torch.float64).view(H, 4) + 0.5)
        fm.vs_stats[1].copy_(torch.arange(H * NB * 5, device=dev, dtype=torch.float64).view(H, NB, 5) + 0.25)
    sentinel = fms[0].es_stats[1].clone(), fms[0].vs_stats[1].clone()
    for update in range(2):
        m, t = _values(K, S, H, I, rng, scaler)
        md, td = _on_device(m, t, case["members"], case["target"], dev)
        ids = np.resize(np.array([2, 0, 2, 0, 2] if update == 0 else [0, 2, 2, 0, 0], dtype=np.int32), S)
        idd = torch.from_numpy(ids).to(dev)
        outs = fms[0].update(md, td, idd, outputs=("energy", "variogram") if update == 0 else ())
        assert fms[1].update(md, td, idd) == {}
        q = FR.accumulate(want_es, mags, want_vs, bound, m, t, ids, scaler, pc, order)
        if update == 0:
            assert set(outs) == {"energy", "variogram"} and outs["variogram"].shape == (S, H, NB, 4)
            es_o, vs_o = outs["energy"].cpu().numpy(), outs["variogram"].cpu().numpy()
            ebar = FR.energy_bar(I, K, 1, q["es"])
            assert np.all(np.abs(es_o - q["es"]) <= ebar), "per-sample energy"
            assert np.array_equal(vs_o[..., 0], q["vs"][..., 0]), "per-sample pair counts"
            assert np.all(np.abs(vs_o[..., 1:] - q["vs"][..., 1:]) <= q["vs_bound"]), "per-sample variogram"
    assert torch.equal(fms[0].es_stats, fms[1].es_stats) and torch.equal(fms[0].vs_stats, fms[1].vs_stats), "not reproducible"
    assert torch.equal(fms[0].es_stats[1], sentinel[0]) and torch.equal(fms[0].vs_stats[1], sentinel[1]), "the never-visited group was touched"
    got_es, got_vs = fms[0].es_stats.cpu().numpy(), fms[0].vs_stats.cpu().numpy()
    got_es[1] = want_es[1] = 0
    got_vs[1] = want_vs[1] = 0
    _check(got_es, got_vs, want_es, mags, want_vs, bound, I, K, 2 * S, repr(case))
    assert got_es[..., 0].sum() == 2 * S * H
    if NB and case["classes"] == "random":
        n_pairs = np.array([(np.triu(pc == c, 1)).sum() for c in range(NB)])
        assert np.array_equal(got_vs[0, 0, :, 1], n_pairs * got_es[0, 0, 0])
        if NB >= 3:
            assert n_pairs[NB - 2] == 0 and (got_vs[:, :, NB - 2, 1:] == 0).all()        # the class that stays empty
        fms[0].es_stats[1].zero_()                                                      # take the sentinel out again
        fms[0].vs_stats[1].zero_()
        out = fms[0].compute()
        assert np.isnan(out["energy_score"][1]).all() and np.isfinite(out["energy_score"][[0, 2]]).all()
        assert out["variogram_score"].shape == (G, H, NB)
    if case["classes"] == "excluded":
        assert (got_vs[..., 1:] == 0).all()
    check_device_errors()                                                               # no id was out of range


def test_two_halves_of_a_batch_accumulate_to_the_whole(dev):
    from src.evaluation.metrics import FieldMetrics
    K, S, H, I, NB = 4, 6, 2, 70, 3
    rng = np.random.default_rng(77)
    pc = _classes(I, NB, "random", rng)
    m, t = _values(K, S, H, I, rng, SCALER)
    md, td = _on_device(m, t, "contiguous", "dataset", dev)
    fm = FieldMetrics(H, I, K, torch.from_numpy(pc).to(dev), NB, 0.5, 1, SCALER, device=dev)
    fm.update(md[:, :3], td[:3])
    fm.update(md[:, 3:], td[3:])
    want_es, mags, want_vs, bound = np.zeros((1, H, 4)), np.zeros((1, H, 4)), np.zeros((1, H, NB, 5)), np.zeros((1, H, NB, 3))
    FR.accumulate(want_es, mags, want_vs, bound, m, t, None, SCALER, pc, 0.5)
    _check(fm.es_stats.cpu().numpy(), fm.vs_stats.cpu().numpy(), want_es, mags, want_vs, bound, I, K, S, "two halves")
    fm.reset()
    assert float(fm.es_stats.abs().sum()) == 0 == float(fm.vs_stats.abs().sum())


def test_a_group_id_out_of_range_is_skipped_and_reported(dev):
    """One sample with id = G (and, in a second object, one with id -1): the other samples are accumulated, the bad sample
    enters no sum, its per-sample rows are not written, and check_device_errors() raises TecmError naming TECM_BAD_GROUP
    once.  An error flag, not a fault."""
    from src.evaluation.metrics import FieldMetrics
    from tecmollm import TecmError, check_device_errors
    check_device_errors()
    rng = np.random.default_rng(12)
    K, S, H, I, G, NB = 8, 5, 3, 70, 3, 2
    pc = _classes(I, NB, "random", rng)
    for bad in (3, -1):
        m, t = _values(K, S, H, I, rng, SCALER)
        md, td = _on_device(m, t, "contiguous", "dataset", dev)
        ids = np.array([0, bad, 1, 2, 0], dtype=np.int32)
        fm = FieldMetrics(H, I, K, torch.from_numpy(pc).to(dev), NB, 0.5, G, SCALER, device=dev)
        outs = fm.update(md, td, torch.from_numpy(ids).to(dev), outputs=("energy", "variogram"))
        want_es, mags, want_vs, bound = np.zeros((G, H, 4)), np.zeros((G, H, 4)), np.zeros((G, H, NB, 5)), np.zeros((G, H, NB, 3))
        FR.accumulate(want_es, mags, want_vs, bound, m, t, ids, SCALER, pc, 0.5)
        _check(fm.es_stats.cpu().numpy(), fm.vs_stats.cpu().numpy(), want_es, mags, want_vs, bound, I, K, S, f"bad id {bad}")
        assert float(fm.es_stats[..., 0].sum()) == 4 * H
        assert torch.isnan(outs["energy"][1]).all() and torch.isnan(outs["variogram"][1]).all()
        assert torch.isfinite(outs["energy"][[0, 2, 3, 4]]).all()
        with pytest.raises(TecmError, match="TECM_BAD_GROUP"):
            check_device_errors()
        check_device_errors()                                              # reported once, then clear


def test_refusals_reach_python(dev):
    from src.evaluation.metrics import FieldMetrics
    pc = torch.zeros(5, 5, dtype=torch.uint8, device=dev)
    for kw in (dict(members=0), dict(members=65), dict(num_classes=17, pair_class=pc), dict(order=0.7),
               dict(num_classes=2), dict(pair_class=pc), dict(pair_class=pc[:4], num_classes=2),
               dict(pair_class=pc.int(), num_classes=2)):
        with pytest.raises(ValueError):
            FieldMetrics(**{**dict(num_horizons=2, num_nodes=5, members=4, device=dev), **kw})
    fm = FieldMetrics(2, 5, 4, device=dev)
    with pytest.raises(ValueError):
        fm.update(torch.zeros(3, 2, 2, 5, device=dev), torch.zeros(2, 2, 5, device=dev))
    with pytest.raises(ValueError):
        fm.update(torch.zeros(4, 2, 2, 5, device=dev), torch.zeros(2, 2, 5, device=dev), outputs=("crps",))
    one = FieldMetrics(2, 5, 1, device=dev)                                  # a point forecast, given as (S, H, N, 1)
    p, t = torch.randn(3, 2, 5, 1, device=dev), torch.randn(3, 2, 5, 1, device=dev)
    a = one.update(p, t, outputs=("energy",))["energy"]
    want = (p.double() - t.double()).squeeze(-1).pow(2).sum(-1).sqrt()
    assert torch.equal(a[..., 1], torch.zeros_like(want)) and torch.allclose(a[..., 0], want, rtol=1e-14) and torch.equal(a[..., 0], a[..., 2])
    out = one.compute()
    assert np.isnan(out["fair_energy_score"]).all() and np.array_equal(out["energy_score"], out["field_error_mean"])


# ------------------------------------------------------------------------------------ shuffled against coherent members
def test_shuffled_members_keep_every_cell_score_and_lose_the_variogram_score(dev):
    """The generator of the host test on the device: `EnsembleMetrics` cannot tell the two ensembles apart, bit for bit;
    the first-class variogram score of the shuffled one is more than 1.5 times the coherent one's."""
    from src.evaluation.metrics import EnsembleMetrics, FieldMetrics
    from tecmollm.fields import pair_classes
    members, shuffled, truth, d = FR.coherent_and_shuffled(0)
    K, S, H, I = members.shape
    pc = torch.from_numpy(pair_classes(d, (0.0, 150.0, 300.0, 600.0, np.inf))).to(dev)
    td = torch.from_numpy(truth).to(dev)
    res = []
    for mem in (members, shuffled):
        md = torch.from_numpy(mem).to(dev)
        em = EnsembleMetrics(H, I, K, 1, SCALER, 1, device=dev)
        fm = FieldMetrics(H, I, K, pc, 4, 0.5, 1, SCALER, device=dev)
        em.update(md, td)
        fm.update(md, td)
        res.append((em.stats.clone(), em.hist.clone(), fm.compute()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    co, sh = res[0][2], res[1][2]
    ratio = sh["variogram_score"].mean(axis=(0, 1)) / co["variogram_score"].mean(axis=(0, 1))
    print("shuffled / coherent variogram score by class:", ratio, "energy score:",
          sh["energy_score"].mean() / co["energy_score"].mean())
    assert ratio[0] > 1.5 and (ratio > 1.0).all()
    assert sh["energy_score"].mean() > co["energy_score"].mean()
    assert np.array_equal(sh["variogram_obs"], co["variogram_obs"]) and np.array_equal(sh["field_error_mean"], co["field_error_mean"])
    assert (sh["variogram_ratio"][..., 0] > co["variogram_ratio"][..., 0]).all()         # rougher at short range


# ------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def tiny(dev):
    from oracle import ref_cpu as R
    from tests.parity import build_model
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=12)
    model = build_model(cfg, R.init_params(cfg, seed=3), dev, "per_timestep").eval()
    return dict(model=model, eid=R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev))


def _spec():
    from tecmollm.fields import FieldSpec, grid_pair_classes
    edges = (0.0, 150.0, 300.0, np.inf)
    return FieldSpec(grid_pair_classes(30.0 + np.arange(3), 100.0 + np.arange(4), edges), edges, 0.5)


def _identical(a, b, where=""):
    """Bit for bit through dicts, lists, arrays and numbers (NaN equal to NaN)."""
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            _identical(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for n, (u, v) in enumerate(zip(a, b)):
            _identical(u, v, f"{where}[{n}]")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    elif isinstance(a, float):
        assert a == b or (a != a and b != b), where
    else:
        assert a == b, where


def _same_old_keys(prob, plain):
    from src.evaluation.metrics import FIELD_KEYS
    assert set(prob) == set(plain) | (set(FIELD_KEYS) - {"count"}) | {"field_count", "field_order", "field_edges_km"}
    _identical({k: prob[k] for k in plain}, plain, "prob")


def test_evaluate_ensemble_with_fields_on_a_tiny_model(dev, golden_dir, tiny, tmp_path):
    """The split, model and settings of tests/test_gpu_ensemble.py's end-to-end test (12 nodes, 24 windows, batch size 5,
    K = 4): every key of the call without `fields` is bit-identical, and the new keys are those of a `FieldMetrics` fed
    `ensemble_members` with the same (seed, chunk)."""
    from src.data.dataset import SlidingWindowSamplerDataset
    from src.evaluation.metrics import FIELD_KEYS, FieldMetrics
    from tecmollm import ensemble as EN
    from tecmollm import evaluate as E
    from tecmollm.fields import write_fields
    g = np.load(os.path.join(golden_dir, "evaluate_split.npz"))
    ds = SlidingWindowSamplerDataset.from_tensors(torch.as_tensor(g["X"]), torch.as_tensor(g["Y"]), torch.as_tensor(g["TF"]),
                                                  int(g["L_in"]), int(g["L_out"]), stride=1, device=dev, mode="test")
    scaler, model, ei, spec = (float(g["mean"]), float(g["scale"])), tiny["model"], tiny["eid"], _spec()
    S, N, H, K = len(ds), 12, 12, 4
    slots = E.window_groups_by_slot(ds)
    kw = dict(members=K, seed=3, scaler=scaler, trim=1, baselines=("mean", "last"), groups=slots, num_groups=12)
    res0, maps0, prob0 = EN.evaluate_ensemble(model, ds, ei, 5, **kw)
    res1, maps1, prob1 = EN.evaluate_ensemble(model, ds, ei, 5, fields=spec, **kw)
    _identical(res1, res0, "results")
    _identical(maps1, maps0, "maps")
    _same_old_keys(prob1, prob0)
    fm = FieldMetrics(H, N, K, torch.from_numpy(spec.pair_class).to(dev), 3, 0.5, 12, scaler, device=dev)
    for ordinal, chunk in enumerate([list(range(a, min(a + 5, S))) for a in range(0, S, 5)]):
        x, tf, y = ds.batch(chunk)
        fm.update(EN.ensemble_members(model, x, tf, ei, K, 3, ordinal), y, slots[chunk])
    want = fm.compute()
    for k in FIELD_KEYS[1:]:
        assert np.array_equal(want[k], prob1[k], equal_nan=True), k
    assert prob1["field_order"] == 0.5 and prob1["field_edges_km"] == [0.0, 150.0, 300.0, float("inf")]
    host = slots.tolist()
    for s in range(12):
        assert (fm.es_stats[s, :, 0] == host.count(s)).all()
        assert np.isfinite(prob1["energy_score"][s]).all() == (host.count(s) > 0)
    seen = [s for s in range(12) if host.count(s)]
    assert (prob1["fair_energy_score"][seen] <= prob1["energy_score"][seen]).all()
    assert (prob1["pairs"][seen].sum(axis=-1) == np.array([host.count(s) for s in seen])[:, None] * 66).all()   # every pair has a class
    paths = write_fields(prob1, str(tmp_path / "out"))
    z = np.load(paths["npz"])
    assert np.array_equal(z["count"], prob1["field_count"]) and np.array_equal(prob1["field_count"], prob1["count"][:, :, 0])
    for k in FIELD_KEYS[1:]:
        assert np.array_equal(z[k], prob1[k], equal_nan=True), k
    with open(paths["csv"], encoding="utf-8") as f:
        assert len(f.read().splitlines()) == 1 + 12 * H * 4


def test_evaluate_analog_ensemble_with_fields(dev):
    """The seasonal record of tests/test_gpu_analog.py (600 steps, 12 nodes), k = 4 analogs: old keys bit-identical, new keys
    those of a `FieldMetrics` fed the analog members batch by batch."""
    import tecmollm
    from src.evaluation.metrics import FIELD_KEYS, FieldMetrics
    from src.models.baselines import AnalogBaseline
    from tests import linear_ref as LR
    from tests.test_gpu_analog import L_OUT, T_ALL, make_dataset
    y = LR.synthetic(T_ALL, 12, 1, seasonal=True)
    full = make_dataset(dev, y)
    n_fit = 2 * len(full) // 3
    ds = make_dataset(dev, y, slice(n_fit, None))
    ana = AnalogBaseline(k=4, device=dev).fit(full, range(n_fit))
    spec, scaler = _spec(), (20.0, 7.0)
    r0, m0, prob0 = tecmollm.evaluate_analog_ensemble(ana, ds, 64, scaler=scaler, trim=1)
    r1, m1, prob1 = tecmollm.evaluate_analog_ensemble(ana, ds, 64, scaler=scaler, trim=1, fields=spec)
    _identical(r1, r0, "results")
    _identical(m1, m0, "maps")
    _same_old_keys(prob1, prob0)
    fm = FieldMetrics(L_OUT, 12, 4, torch.from_numpy(spec.pair_class).to(dev), 3, 0.5, 1, scaler, device=dev)
    for a in range(0, len(ds), 64):
        chunk = list(range(a, min(a + 64, len(ds))))
        fm.update(ana.members(ds, chunk), ds.batch(chunk)[2])
    want = fm.compute()
    for k in FIELD_KEYS[1:]:
        assert np.array_equal(want[k], prob1[k], equal_nan=True), k
    assert (prob1["field_count"] == len(ds)).all() and np.isfinite(prob1["variogram_score"]).all() and (prob1["energy_score"] > 0).all()
