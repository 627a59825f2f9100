"""GPU tests of the member reordering: the kernel (tecm_member_reorder) through `reorder_members` against the numpy restatement
(tests/coherence_ref.py), with both template sources, every stride layout the callers produce, in-place use, hard values,
bad dates, refusals; then what it is for -- `evaluate_analog_ensemble(..., reorder=)`, the coherence gain on the generator of
the field tests, and `evaluate_quantile_ensemble`.

The kernel moves bit patterns and compares: every comparison with the restatement is exact (np.array_equal on the uint32
view of the floats, so the sign of a zero and the payload of a NaN count; np.array_equal on the ranks).  There is no
tolerance in this file.  The two bars of the coherence test (a factor of 1.5 on the first-class variogram score, a lower
energy score) are those of tests/test_host_coherence.py."""
import numpy as np
import pytest
import torch

from tests import coherence_ref as CR
from tests import fields_ref as FR

pytestmark = pytest.mark.gpu

SCALER = (21.5, 9.25)
BASE = dict(K=8, S=2, H=3, N=65)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).sum()), "elements differ")


def _cases():
    out = [dict(BASE)]
    for key, vals in (("K", (2, 3, 5, 16, 17, 33, 64)), ("N", (1, 63, 64, 257)), ("H", (1,)), ("S", (1,))):
        out += [dict(BASE, **{key: v}) for v in vals]
    return out


def _draw(rng, shape, ties):
    """float32 values; with `ties` small integers, so that most cells hold equal members."""
    if ties:
        return rng.integers(-1, 2, size=shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


# ------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("case", _cases(), ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items() if BASE[k] != v) or "base")
def test_shapes_match_the_restatement_with_both_template_sources(dev, case):
    """One axis at a time around K = 8, S = 2, H = 3, N = 65: every padded size and K one past a bucket (3, 5, 17, 33), N of one
    lane, one short of a tile, a tile, one over and four tiles and a lane, H = 1, S = 1.  Values with ties (integers in
    [-1, 1]) against a continuous template and the other way round; out and ranks, member template and dated rows."""
    from tecmollm import check_device_errors, reorder_members
    K, S, H, N = (case[k] for k in "KSHN")
    rng = np.random.default_rng(K * 1000 + S * 100 + H * 10 + N)
    for ties_v, ties_t in ((False, False), (True, False), (False, True)):
        v, t = _draw(rng, (K, S, H, N), ties_v), _draw(rng, (K, S, H, N), ties_t)
        want, want_r = CR.reorder(v, t, want_ranks=True)
        got, got_r = reorder_members(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), return_ranks=True)
        assert got.shape == (K, S, H, N) and got.dtype == torch.float32 and got.is_contiguous() and got_r.dtype == torch.uint8
        _same_bits(got, want, ("members", case, ties_v, ties_t))
        assert np.array_equal(got_r.cpu().numpy(), want_r), ("ranks", case)
        T = H + 9
        series = _draw(rng, (T, N), ties_t)
        rows = rng.integers(0, T - H + 1, size=(S, K)).astype(np.int32)
        want, want_r = CR.reorder_dated(v, series, rows, want_ranks=True)
        got, got_r = reorder_members(torch.from_numpy(v).to(dev), torch.from_numpy(series).to(dev),
                                     rows=torch.from_numpy(rows).to(dev), return_ranks=True)
        _same_bits(got, want, ("dated members", case, ties_v, ties_t))
        assert np.array_equal(got_r.cpu().numpy(), want_r), ("dated ranks", case)
    check_device_errors()


# ------------------------------------------------------------------------------------ strides and in-place use
def test_strided_operands_are_read_and_written_where_they_lie(dev):
    """values as the stack of K model-shaped outputs -- storage (K, B, N, L_out), seen as (K, B, L_out, N, 1) --, the template
    as every second member, sample and node of a larger tensor, out (a) new, (b) a slice of a larger tensor whose other
    elements must survive, (c) the values themselves."""
    from tecmollm import reorder_members
    K, S, H, N = 5, 3, 4, 70
    rng = np.random.default_rng(3)
    v, t = _draw(rng, (K, S, H, N), False), _draw(rng, (K, S, H, N), True)
    want = CR.reorder(v, t)
    store = torch.from_numpy(np.ascontiguousarray(v.transpose(0, 1, 3, 2))).to(dev)            # (K, B, N, L_out)
    vd = store.permute(0, 1, 3, 2).unsqueeze(-1)
    assert vd.shape == (K, S, H, N, 1) and vd.stride(2) == 1 and vd.stride(3) == H
    big = torch.full((2 * K, 2 * S, H, 2 * N + 1), 7.0, device=dev)
    td = big[::2, 1::2, :, 1::2][..., :N]
    td.copy_(torch.from_numpy(t).to(dev))
    assert not td.is_contiguous() and td.shape == (K, S, H, N)
    got = reorder_members(vd, td)
    assert got.shape == (K, S, H, N, 1)
    _same_bits(got.squeeze(-1), want, "new out")
    frame = torch.full((K, S + 2, H, N + 3), -5.0, device=dev)
    o = frame[:, 1:S + 1, :, 2:N + 2]
    assert reorder_members(vd, td, out=o) is o
    _same_bits(o, want, "sliced out")
    frame[:, 1:S + 1, :, 2:N + 2] = -5.0
    assert bool((frame == -5.0).all()), "out wrote outside its view"
    _same_bits(store.permute(0, 1, 3, 2), v, "the values were modified")
    back, ranks = reorder_members(vd, td, out=vd, return_ranks=True)                            # in place, permuted strides
    assert back is vd
    _same_bits(store.permute(0, 1, 3, 2), want, "in place")
    assert np.array_equal(ranks.cpu().numpy(), CR.ranks(t).astype(np.uint8))
    assert bool((big[1::2] == 7.0).all()) and bool((big[:, ::2] == 7.0).all()), "the template's surroundings were modified"


# ------------------------------------------------------------------------------------ dated template
@pytest.mark.parametrize("layout", ["time-major", "node-major"])
def test_dated_template_reads_the_archive_in_place_and_refuses_bad_dates(dev, layout):
    """A (T, N) series and the node-major (N, Ty) archive of a fitted AnalogBaseline (seen as its (Ty, N) transpose): a row at
    T - H is served; a row at T - H + 1 and a row of -1 each give NaN members and rank 255 for THAT sample only, and
    `check_device_errors` reports TECM_BAD_ROW once.  The archive lies at the end of a larger allocation filled with NaN
    on both sides, so a read outside it would change the result."""
    from tecmollm import TecmError, check_device_errors, reorder_members
    check_device_errors()
    K, S, H, N, T = 6, 5, 3, 67, 40
    rng = np.random.default_rng(11)
    series = _draw(rng, (T, N), False)
    v = _draw(rng, (K, S, H, N), False)
    pad = torch.full((T * N + 2 * 256,), float("nan"), device=dev)
    body = pad[256:256 + T * N]
    if layout == "time-major":
        sd = body.view(T, N)
        sd.copy_(torch.from_numpy(series).to(dev))
    else:
        body.view(N, T).copy_(torch.from_numpy(np.ascontiguousarray(series.T)).to(dev))
        sd = body.view(N, T).t()
        assert sd.stride() == (1, T)
    rows = rng.integers(0, T - H + 1, size=(S, K)).astype(np.int32)
    rows[0, 2] = T - H                                                    # the last row that has H rows behind it
    rows[4, 0] = 0
    vd, rd = torch.from_numpy(v).to(dev), torch.from_numpy(rows).to(dev)
    got, ranks = reorder_members(vd, sd, rows=rd, return_ranks=True)
    want, want_r = CR.reorder_dated(v, series, rows, want_ranks=True)
    assert np.isfinite(want).all()
    _same_bits(got, want, "good dates")
    assert np.array_equal(ranks.cpu().numpy(), want_r)
    check_device_errors()
    for bad_row, bad_value in ((1, T - H + 1), (3, -1)):
        rows2 = rows.copy()
        rows2[bad_row, K - 1] = bad_value
        got, ranks = reorder_members(vd, sd, rows=torch.from_numpy(rows2).to(dev), return_ranks=True)
        want, want_r = CR.reorder_dated(v, series, rows2, want_ranks=True)
        assert np.isnan(want[:, bad_row]).all() and np.isfinite(np.delete(want, bad_row, axis=1)).all()
        assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), bad_value
        _same_bits(np.delete(got.cpu().numpy(), bad_row, axis=1), np.delete(want, bad_row, axis=1), bad_value)
        assert np.array_equal(ranks.cpu().numpy(), want_r), bad_value
        with pytest.raises(TecmError, match="TECM_BAD_ROW"):
            check_device_errors()
        check_device_errors()                                             # reported once, then clear


# ------------------------------------------------------------------------------------ hard values
def test_ties_zeros_infinities_and_nans_follow_the_total_order(dev):
    """Templates of two and three distinct integers (most members tied), an all-equal template (the output is the values
    sorted), and both operands seeded with -0.0, +0.0, both infinities, NaNs with different payloads and denormals; values
    whose last members are NaN, as the analog members are where fewer than K analogs were admitted."""
    from tecmollm import reorder_members
    K, S, H, N = 16, 2, 2, 130
    rng = np.random.default_rng(8)
    special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fc01234, 0x7f800001,
                        0x00000001, 0x80000001, 0x007fffff, 0x3f800000, 0xbf800000], dtype=np.uint32).view(np.float32)

    def hard(shape):
        a = _draw(rng, shape, False)
        pick = rng.random(shape) < 0.5
        a[pick] = special[rng.integers(0, special.size, size=int(pick.sum()))]
        return a

    v = hard((K, S, H, N))
    two = rng.integers(0, 2, size=v.shape).astype(np.float32)
    three = rng.integers(-1, 2, size=v.shape).astype(np.float32)
    flat = np.full(v.shape, np.float32(3.5))
    tail = _draw(rng, v.shape, False)
    count = rng.integers(0, K + 1, size=(S, H, N))
    tail[np.arange(K).reshape(K, 1, 1, 1) >= count[None]] = np.nan                          # members count .. K - 1 are NaN
    for name, values, template in (("two values", v, two), ("three values", v, three), ("all equal", v, flat),
                                   ("hard template", v, hard(v.shape)), ("hard both", hard(v.shape), hard(v.shape)),
                                   ("nan tail", tail, _draw(rng, v.shape, False)), ("nan tail, ties", tail, two)):
        want, want_r = CR.reorder(values, template, want_ranks=True)
        got, got_r = reorder_members(torch.from_numpy(values).to(dev), torch.from_numpy(template).to(dev), return_ranks=True)
        _same_bits(got, want, name)
        assert np.array_equal(got_r.cpu().numpy(), want_r), name
        assert np.array_equal(np.sort(_bits(got), axis=0), np.sort(_bits(values), axis=0)), name    # a permutation of the bits
    got = reorder_members(torch.from_numpy(v).to(dev), torch.from_numpy(flat).to(dev))
    order = np.argsort(v, axis=0, kind="stable")
    _same_bits(got, np.take_along_axis(v.view(np.uint32), order, axis=0).view(np.float32), "sorted")
    got = reorder_members(torch.from_numpy(tail).to(dev), torch.from_numpy(_draw(rng, v.shape, False)).to(dev))
    assert np.array_equal(np.isnan(got.cpu().numpy()).sum(axis=0), K - count)               # every NaN is still there


def test_two_calls_give_identical_bits(dev):
    from tecmollm import reorder_members
    rng = np.random.default_rng(2)
    v, t = torch.from_numpy(_draw(rng, (16, 4, 12, 300), True)).to(dev), torch.from_numpy(_draw(rng, (16, 4, 12, 300), True)).to(dev)
    a, ra = reorder_members(v, t, return_ranks=True)
    b, rb = reorder_members(v, t, return_ranks=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ra, rb)


# ------------------------------------------------------------------------------------ refusals
def test_refusals_reach_python(dev):
    from tecmollm import TecmError, _lib, ops, reorder_members
    v = torch.zeros(4, 2, 3, 5, device=dev)
    t = torch.ones(4, 2, 3, 5, device=dev)
    for values, template, kw in (
            (v[:1], t[:1], {}),                                               # K = 1
            (torch.zeros(65, 1, 1, 2, device=dev), torch.zeros(65, 1, 1, 2, device=dev), {}),          # K = 65
            (v, t[:3], {}), (v, t[:, :1], {}), (v, t[..., :4], {}), (v, t[0], {}),                      # shapes
            (v.double(), t, {}), (v, t.double(), {}), (v, t.cpu(), {}), (v.cpu(), t.cpu(), {}),         # dtype, device
            (v, t, dict(out=torch.zeros(4, 2, 3, 6, device=dev))), (v, t, dict(out=torch.zeros(4, 2, 3, 5))),
            (v, t, dict(out=torch.zeros(4, 2, 3, 5, device=dev, dtype=torch.float64))),
            (v, t, dict(out=t)),                                              # out is the template
            (v, t, dict(out=torch.zeros(1, 2, 3, 5, device=dev).expand(4, 2, 3, 5))),                   # cells share storage
            (v, torch.zeros(9, 5, device=dev), dict(rows=torch.zeros(2, 4, device=dev, dtype=torch.int64))),
            (v, torch.zeros(9, 5, device=dev), dict(rows=torch.zeros(2, 3, device=dev, dtype=torch.int32))),
            (v, torch.zeros(9, 4, device=dev), dict(rows=torch.zeros(2, 4, device=dev, dtype=torch.int32))),
            (v, torch.zeros(2, 5, device=dev), dict(rows=torch.zeros(2, 4, device=dev, dtype=torch.int32))),   # T < H
            (v, t, dict(rows=torch.zeros(2, 4, device=dev, dtype=torch.int32)))):
        with pytest.raises(ValueError):
            reorder_members(values, template, **kw)
    buf = torch.zeros(4 * 2 * 3 * 5 + 7, device=dev)
    values, shifted = buf[:120].view(4, 2, 3, 5), buf[7:127].view(4, 2, 3, 5)
    with pytest.raises(ValueError, match="overlaps values"):
        reorder_members(values, t, out=shifted)                               # a partial overlap
    with pytest.raises(ValueError, match="overlaps values"):
        reorder_members(values, t, out=buf[:120].view(2, 4, 3, 5).permute(1, 0, 2, 3))   # the same storage under other strides
    assert reorder_members(values, t, out=values) is values                   # the same view: allowed
    # the library applies the same rules to a caller that goes round the wrapper
    for values, template, out in ((values, t, shifted), (v, t, t), (v[:1], t[:1], torch.zeros(1, 2, 3, 5, device=dev))):
        with pytest.raises(TecmError, match="tecm_member_reorder"):
            ops.member_reorder(values, template, out)
    with pytest.raises(TecmError, match="error word"):
        ops.member_reorder(v, torch.zeros(9, 5, device=dev), torch.zeros_like(v), torch.zeros(2, 4, device=dev, dtype=torch.int32))
    assert _lib.TECM_REORDER_MAX_GRID == 65535


# ------------------------------------------------------------------------------------ what it is for
def _identical(a, b, where=""):
    """Bit for bit through dicts, lists, arrays and numbers (NaN equal to NaN); returns the paths that differ."""
    if type(a) is not type(b):
        return [where]
    if isinstance(a, dict):
        if list(a) != list(b):
            return [where + "/keys"]
        return [p for k in a for p in _identical(a[k], b[k], f"{where}/{k}")]
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            return [where + "/len"]
        return [p for n, (u, v) in enumerate(zip(a, b)) for p in _identical(u, v, f"{where}[{n}]")]
    if isinstance(a, np.ndarray):
        return [] if a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() else [where]
    if isinstance(a, float):
        return [] if a == b or (a != a and b != b) else [where]
    return [] if a == b else [where]


def _field_keys():
    from src.evaluation.metrics import FIELD_KEYS
    return (set(FIELD_KEYS) - {"count"}) | {"field_count", "field_order", "field_edges_km"}


def _spec():
    from tecmollm.fields import FieldSpec, grid_pair_classes
    edges = (0.0, 150.0, 300.0, np.inf)
    return FieldSpec(grid_pair_classes(30.0 + np.arange(3), 100.0 + np.arange(4), edges), edges, 0.5)


def test_analog_ensemble_keeps_every_per_cell_score_under_the_schaake_shuffle(dev):
    """The seasonal record of tests/test_gpu_analog.py (600 steps, 12 nodes), k = 4 analogs, the Schaake dates from the first
    400 rows: `results`, `maps` and every per-cell key of `prob` are bit-identical with and without `reorder=`; the field
    keys are those of a `FieldMetrics` fed `AnalogBaseline.members(..., reorder=)` batch by batch, and they differ."""
    import tecmollm
    from src.evaluation.metrics import FIELD_KEYS
    from src.models.baselines import AnalogBaseline
    from tests import linear_ref as LR
    from tests.test_gpu_analog import L_OUT, T_ALL, make_dataset
    y = LR.synthetic(T_ALL, 12, 1, seasonal=True)
    full = make_dataset(dev, y)
    n_fit = 2 * len(full) // 3
    ds = make_dataset(dev, y, slice(n_fit, None))
    ana = AnalogBaseline(k=4, device=dev).fit(full, range(n_fit))
    tpl = tecmollm.SchaakeTemplate(make_dataset(dev, y, slice(0, 400), mode="train"), 4, seed=5)
    spec, scaler = _spec(), (20.0, 7.0)
    r0, m0, p0 = tecmollm.evaluate_analog_ensemble(ana, ds, 64, scaler=scaler, trim=1, fields=spec)
    r1, m1, p1 = tecmollm.evaluate_analog_ensemble(ana, ds, 64, scaler=scaler, trim=1, fields=spec, reorder=tpl)
    assert _identical(r1, r0, "results") == [] and _identical(m1, m0, "maps") == []
    assert set(p1) == set(p0)
    per_cell = [k for k in p0 if k not in _field_keys()]
    assert "crps" in per_cell and "rank_histogram" in per_cell
    assert _identical({k: p1[k] for k in per_cell}, {k: p0[k] for k in per_cell}, "prob") == []
    assert np.array_equal(p1["field_count"], p0["field_count"]) and np.array_equal(p1["variogram_obs"], p0["variogram_obs"])
    assert not np.array_equal(p1["variogram_score"], p0["variogram_score"]) and not np.array_equal(p1["energy_score"], p0["energy_score"])
    fm = spec.metrics(L_OUT, 12, 4, 1, scaler, dev)
    for a in range(0, len(ds), 64):
        chunk = list(range(a, min(a + 64, len(ds))))
        plain, mem = ana.members(ds, chunk), ana.members(ds, chunk, reorder=tpl)
        assert torch.equal(torch.sort(plain, dim=0).values, torch.sort(mem, dim=0).values) and not torch.equal(plain, mem)
        want = CR.reorder_dated(plain.cpu().numpy(), tpl.series.cpu().numpy(), tpl.rows(ds, chunk).cpu().numpy())
        _same_bits(mem, want, "members(..., reorder=)")
        fm.update(mem, ds.batch(chunk)[2])
    want = fm.compute()
    for k in FIELD_KEYS[1:]:
        assert np.array_equal(want[k], p1[k], equal_nan=True), k
    print("analog first-class variogram score, per-node / Schaake:", p0["variogram_score"][0, :, 0].mean(),
          p1["variogram_score"][0, :, 0].mean(), "energy score:", p0["energy_score"].mean(), p1["energy_score"].mean())


def test_reordered_shuffled_members_regain_the_variogram_score_on_the_device(dev):
    """`fields_ref.coherent_and_shuffled(0)`: the shuffled members reordered by the kernel with an independent coherent draw
    (seed 100) as template -- `EnsembleMetrics` cannot tell the three ensembles apart, bit for bit; the first-class variogram
    score of the shuffled one is more than 1.5 times the reordered one's and its energy score is higher; and reordering the
    shuffled members with the original ones as template gives the original ones back."""
    from src.evaluation.metrics import EnsembleMetrics, FieldMetrics
    from tecmollm import reorder_members
    from tecmollm.fields import pair_classes
    members, shuffled, truth, d = FR.coherent_and_shuffled(0)
    template = FR.coherent_and_shuffled(100)[0]
    K, S, H, I = members.shape
    pc = torch.from_numpy(pair_classes(d, (0.0, 150.0, 300.0, 600.0, np.inf))).to(dev)
    td = torch.from_numpy(truth).to(dev)
    md, sd = torch.from_numpy(members).to(dev), torch.from_numpy(shuffled).to(dev)
    rd = reorder_members(sd, torch.from_numpy(template).to(dev))
    _same_bits(rd, CR.reorder(shuffled, template), "reordered")
    _same_bits(reorder_members(sd, md), members, "the original members as template")
    res = {}
    for name, mem in (("coherent", md), ("shuffled", sd), ("reordered", rd)):
        em = EnsembleMetrics(H, I, K, 1, SCALER, 1, device=dev)
        fm = FieldMetrics(H, I, K, pc, 4, 0.5, 1, SCALER, device=dev)
        em.update(mem, td)
        fm.update(mem, td)
        res[name] = (em.stats.clone(), em.hist.clone(), fm.compute())
    for name in ("shuffled", "reordered"):
        assert torch.equal(res[name][0], res["coherent"][0]) and torch.equal(res[name][1], res["coherent"][1]), name
    vs = {name: r[2]["variogram_score"].mean(axis=(0, 1))[0] for name, r in res.items()}
    es = {name: r[2]["energy_score"].mean() for name, r in res.items()}
    print("first-class variogram score:", vs, "energy score:", es)
    assert vs["shuffled"] > 1.5 * vs["reordered"]
    assert es["reordered"] < es["shuffled"]


@pytest.fixture(scope="module")
def split(dev, golden_dir):
    import os
    from oracle import ref_cpu as R
    from src.data.dataset import SlidingWindowSamplerDataset
    from tecmollm import QuantileModel, quantile_config
    from tests.parity import build_model
    taus = (0.1, 0.5, 0.9)
    cfg = quantile_config(R.default_config(L_in=16, L_out=12, num_nodes=12), taus)
    model = build_model(cfg, R.init_params(cfg, seed=3), dev, "per_timestep")
    g = np.load(os.path.join(golden_dir, "evaluate_split.npz"))
    ds = SlidingWindowSamplerDataset.from_tensors(torch.as_tensor(g["X"]), torch.as_tensor(g["Y"]), torch.as_tensor(g["TF"]),
                                                  int(g["L_in"]), int(g["L_out"]), stride=1, device=dev, mode="test")
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev)
    return QuantileModel(model, taus, 12).eval(), ds, ei, (float(g["mean"]), float(g["scale"]))


def test_quantile_model_scored_as_an_ensemble_of_maps(dev, split):
    """12 nodes, 24 windows, batch size 5, an untrained three-level model, K = 4 members: with a SchaakeTemplate, an
    EccTemplate and None the shapes and keys are those of `evaluate_ensemble`, the per-cell entries of `prob` are identical
    across the three, "TEC-MoLLM" is `evaluate_split(qmodel, ...)`'s entry, and the members of one batch are
    `quantile_members` of the model's levels reordered by the restatement."""
    from src.evaluation.metrics import ENSEMBLE_KEYS
    from tecmollm import (EccTemplate, SchaakeTemplate, calibrate_cqr, evaluate_quantile_ensemble, quantile_members,
                          reorder_members)
    from tecmollm import evaluate as E
    qmodel, ds, ei, scaler = split
    S, N, H, K = len(ds), 12, 12, 4
    slots = (torch.arange(S, device=dev) % 3).to(torch.int32)
    spec = _spec()
    templates = {"schaake": SchaakeTemplate(ds, K, seed=1, same_slot=False, min_gap=1), "ecc": EccTemplate(qmodel, K, seed=2),
                 "none": None}
    kw = dict(members=K, scaler=scaler, trim=1, groups=slots, num_groups=3, fields=spec)
    out = {name: evaluate_quantile_ensemble(qmodel, ds, ei, 5, tpl, **kw) for name, tpl in templates.items()}
    want_res = E.evaluate_split(qmodel, ds, ei, 5, scaler=scaler, baselines=())
    want_maps = E.evaluate_maps(qmodel, ds, ei, 5, scaler=scaler, baselines=(), groups=slots, num_groups=3)[1]
    for name, (res, maps, prob) in out.items():
        assert list(res) == ["TEC-MoLLM"] == list(maps), name
        assert _identical(res, want_res, "results") == [] and _identical(maps, want_maps, "maps") == [], name
        assert set(prob) == set(ENSEMBLE_KEYS) | {"nominal_coverage", "rank_histogram", "by_group"} | _field_keys(), name
        assert prob["crps"].shape == (3, H, N) and prob["rank_histogram"].shape == (3, H, K + 1)
        assert prob["count"].sum() == S * H * N and np.isfinite(prob["crps"]).all() and np.isfinite(prob["energy_score"]).all()
    per_cell = [k for k in out["none"][2] if k not in _field_keys()]
    for name in ("schaake", "ecc"):
        a, b = ({k: out[n][2][k] for k in per_cell} for n in (name, "none"))
        assert _identical(a, b, f"prob[{name}]") == []
        assert not np.array_equal(out[name][2]["variogram_score"], out["none"][2]["variogram_score"]), name
    # one batch by hand
    with torch.no_grad():
        chunk = list(range(5, 10))
        x, tf, _ = ds.batch(chunk)
        mem = quantile_members(qmodel.quantiles(x, tf, ei), qmodel.taus, K)
        assert mem.shape == (K, 5, H, N) and bool((mem[1:] >= mem[:-1]).all())
        _same_bits(mem, CR.quantile_members(qmodel.quantiles(x, tf, ei).cpu().numpy(), qmodel.taus, K), "quantile_members")
        tpl = templates["schaake"]
        got = reorder_members(mem, tpl.series, rows=tpl.rows(ds, chunk))
        _same_bits(got, CR.reorder_dated(mem.cpu().numpy(), tpl.series.cpu().numpy(), tpl.rows(ds, chunk).cpu().numpy()), "schaake batch")
        raw = templates["ecc"].members(x, tf, ei, 1)
        assert raw.shape == mem.shape
        _same_bits(templates["ecc"].apply_(mem.clone(), ds, chunk, x=x, tf=tf, edge_index=ei, chunk=1),
                   CR.reorder(mem.cpu().numpy(), raw.cpu().numpy()), "ecc batch")
    # calibrated levels widen the ensemble; a template of another size is refused
    iv = calibrate_cqr(qmodel, ds, ei, 5, pair=(0.1, 0.9), scaler=scaler, groups=slots, num_groups=3)
    wide = evaluate_quantile_ensemble(qmodel, ds, ei, 5, None, intervals=iv, **kw)[2]
    assert iv.finite and not np.array_equal(wide["spread"], out["none"][2]["spread"])
    if (iv.offset > 0).all():                                              # every cell under-dispersed: every member moves outward
        assert wide["spread"].mean() > out["none"][2]["spread"].mean()
    with pytest.raises(ValueError, match="exactly K"):
        evaluate_quantile_ensemble(qmodel, ds, ei, 5, SchaakeTemplate(ds, 5, same_slot=False, min_gap=1), **kw)
