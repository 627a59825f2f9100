"""Host tests of the member reordering: the numpy restatement (tests/coherence_ref.py) on its defining properties and on the
property that motivates the feature -- per-node-shuffled members reordered by an independent coherent template regain the
short-range variogram score --, the date rule of `SchaakeTemplate`, `quantile_members`, and the binding.  No GPU; only the last
test loads the library."""
import os

import numpy as np
import pytest
import torch

from tests import coherence_ref as CR
from tests import fields_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tec-mollm_amd", "tecmollm", "libtecmollm_hip.so")
SCALER = (21.5, 9.25)


@pytest.fixture(scope="module")
def generated():
    """(members, shuffled, truth, distances) of the generator of the field tests, computed once per (seed, K)."""
    cache = {}

    def get(seed, K=8):
        if (seed, K) not in cache:
            cache[(seed, K)] = FR.coherent_and_shuffled(seed, K=K)
        return cache[(seed, K)]
    return get


# ------------------------------------------------------------------------------------ the restatement
def test_reference_output_is_a_permutation_of_every_cell_and_ranks_are_permutations(generated):
    members, shuffled, _, _ = generated(0)
    template = generated(100)[0]
    out, r = CR.reorder(shuffled, template, want_ranks=True)
    K = members.shape[0]
    assert out.shape == shuffled.shape and out.dtype == np.float32 and r.dtype == np.uint8
    assert np.array_equal(np.sort(out.view(np.uint32), axis=0), np.sort(shuffled.view(np.uint32), axis=0))
    assert np.array_equal(np.sort(r, axis=0), np.broadcast_to(np.arange(K, dtype=np.uint8).reshape(K, 1, 1, 1), r.shape))
    # the member that holds the template's smallest value holds the smallest value
    assert np.array_equal(np.argmin(out, axis=0), np.argmin(template, axis=0))
    assert np.array_equal(np.argmax(out, axis=0), np.argmax(template, axis=0))


def test_reference_gives_the_original_members_back(generated):
    for seed in range(4):
        members, shuffled, _, _ = generated(seed)
        assert np.array_equal(CR.reorder(shuffled, members).view(np.uint32), members.view(np.uint32))


def test_reference_total_order_on_ties_zeros_and_nans():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    other = np.array([0x7fc00123], dtype=np.uint32).view(np.float32)[0]          # a NaN with a payload
    v = np.array([3.0, -0.0, nan, 0.0, other, -inf, 1.0], dtype=np.float32).reshape(7, 1, 1, 1)
    # sorted by the contract: -inf, -0.0 (index 1), 0.0 (index 3), 1.0, 3.0, nan (index 2), other (index 4)
    t = np.array([5.0, 5.0, nan, -0.0, 0.0, inf, nan], dtype=np.float32).reshape(7, 1, 1, 1)
    # positions of t: -0.0 (3) -> 0, 0.0 (4) -> 1, 5.0 (0) -> 2, 5.0 (1) -> 3, inf (5) -> 4, nan (2) -> 5, nan (6) -> 6
    out, r = CR.reorder(v, t, want_ranks=True)
    assert r.ravel().tolist() == [2, 3, 5, 0, 1, 4, 6]
    want = np.array([0.0, 1.0, nan, -inf, -0.0, 3.0, other], dtype=np.float32)
    assert np.array_equal(out.ravel().view(np.uint32), want.view(np.uint32))
    flat = CR.reorder(v, np.zeros_like(v))                                         # an all-equal template: the values sorted
    want = np.array([-inf, -0.0, 0.0, 1.0, 3.0, nan, other], dtype=np.float32)
    assert np.array_equal(flat.ravel().view(np.uint32), want.view(np.uint32))


def test_reference_dated_template_gathers_rows_and_marks_bad_samples():
    rng = np.random.default_rng(5)
    T, I, S, K, H = 20, 7, 4, 3, 3
    series = rng.standard_normal((T, I)).astype(np.float32)
    rows = rng.integers(0, T - H + 1, size=(S, K)).astype(np.int32)
    rows[0, 0], rows[1, 2], rows[2, 1] = T - H, T - H + 1, -1
    t, bad = CR.dated_template(series, rows, H)
    assert bad.tolist() == [False, True, True, False]
    assert np.array_equal(t[0, 0], series[T - H:]) and np.array_equal(t[2, 3, 1], series[rows[3, 2] + 1])
    v = rng.standard_normal((K, S, H, I)).astype(np.float32)
    out, r = CR.reorder_dated(v, series, rows, want_ranks=True)
    assert np.isnan(out[:, bad]).all() and (r[:, bad] == 255).all() and np.isfinite(out[:, ~bad]).all()
    assert np.array_equal(out[:, ~bad], CR.reorder(v, t)[:, ~bad])


# ------------------------------------------------------------------------------------ the motivating property
@pytest.mark.parametrize("K", [8, 16])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_reordering_by_an_independent_coherent_template_regains_the_variogram_score(generated, seed, K):
    """9 x 13 grid, 500 km correlation range: the per-node-shuffled members, reordered with K coherent maps of an independent
    draw (seed + 100) as template, against the shuffled ones -- the pooled first-class (pairs <= 150 km) variogram score of the
    shuffled members is more than 1.5 times the reordered ones' (the bar tests/test_gpu_fields.py uses for the inverse
    statement; measured 1.74 to 2.01 with the scaler of this file), and the energy score drops in every case."""
    from tecmollm.fields import pair_classes
    members, shuffled, truth, d = generated(seed, K)
    template = generated(seed + 100, K)[0]
    reordered = CR.reorder(shuffled, template)
    pc = pair_classes(d, (0.0, 150.0, 300.0, 600.0, np.inf))
    q = {name: FR.per_sample(m, truth, SCALER, pc, 4, 0.5) for name, m in
         (("coherent", members), ("shuffled", shuffled), ("reordered", reordered))}
    vs = {name: v["vs"][..., 0, 1].sum() for name, v in q.items()}
    es = {name: (v["es"][..., 0] - v["es"][..., 1] / (K * K)).mean() for name, v in q.items()}
    print(f"seed {seed} K {K}: first-class variogram score shuffled / reordered = {vs['shuffled'] / vs['reordered']:.3f}, "
          f"reordered / coherent = {vs['reordered'] / vs['coherent']:.3f}; energy score shuffled {es['shuffled']:.3f}, "
          f"reordered {es['reordered']:.3f}, coherent {es['coherent']:.3f}")
    assert vs["shuffled"] > 1.5 * vs["reordered"]
    assert es["reordered"] < es["shuffled"]
    assert np.array_equal(np.sort(reordered, axis=0), np.sort(shuffled, axis=0))      # the margins did not move


# ------------------------------------------------------------------------------------ the Schaake dates
class _Record:
    pass


def _record(T=400, N=5, L_in=6, L_out=4, slots_known=None, series=True, seed=0):
    """A CPU stand-in for a window dataset: the attributes `SchaakeTemplate` reads."""
    g = torch.Generator().manual_seed(seed)
    ds = _Record()
    ds.L_in, ds.L_out = L_in, L_out
    rows_x = T if slots_known is None else slots_known
    ds.time_features = torch.stack([torch.arange(rows_x) % 12, torch.zeros(rows_x)], dim=1).float()
    ds.X = torch.zeros(rows_x, 1, N, 1)
    if series:
        ds.Ys = torch.randn(T, 1, N, generator=g)
    else:
        ds.Y = torch.randn(T, 1, N, L_out, generator=g)
    ds.sample_indices = list(range(0, rows_x - L_in - L_out + 1))
    ds.num_samples = len(ds.sample_indices)
    return ds


def test_schaake_dates_obey_slot_gap_range_and_distinctness():
    from tecmollm.coherence import SchaakeTemplate
    train, test = _record(seed=1), _record(T=90, seed=2)
    for kw in (dict(), dict(min_gap=1), dict(min_gap=13), dict(same_slot=False), dict(seed=9)):
        tpl = SchaakeTemplate(train, 8, **kw)
        gap = kw.get("min_gap", train.L_out)
        assert tpl.series.shape == (400, 5) and tpl.first_row == 0 and tpl.num_rows == 400
        for index in (0, 1, 17, test.num_samples - 1):
            dates = tpl.dates(test, index)
            assert dates.dtype == np.int32 and dates.shape == (8,)
            assert (dates >= 0).all() and (dates + train.L_out <= 400).all()
            srt = np.sort(dates)
            assert (np.diff(srt) >= gap).all()                          # pairwise apart, hence distinct
            slot = int(test.time_features[test.sample_indices[index] + test.L_in, 0])
            if kw.get("same_slot", True):
                assert (train.time_features[dates.astype(np.int64), 0].numpy() == slot).all()
            want = CR.schaake_dates(400, 0, train.L_out, train.time_features[:, 0].numpy(), slot, kw.get("same_slot", True), 8,
                                    gap, kw.get("seed", 0), index)
            assert np.array_equal(dates, want)
    a, b = SchaakeTemplate(train, 8, seed=0).dates(test, 3), SchaakeTemplate(train, 8, seed=1).dates(test, 3)
    assert not np.array_equal(a, b)


def test_schaake_dates_do_not_depend_on_batch_size_or_order():
    from tecmollm.coherence import SchaakeTemplate
    train, test = _record(seed=1), _record(T=90, seed=2)
    tpl = SchaakeTemplate(train, 4, seed=3)
    idx = list(range(16))
    whole = tpl.rows(test, idx)
    assert whole.dtype == torch.int32 and whole.shape == (16, 4) and whole.device == tpl.series.device
    ones = torch.cat([tpl.rows(test, [i]) for i in idx])
    assert torch.equal(whole, ones)
    perm = [5, 0, 15, 3, 9, 1, 14, 2, 8, 4, 13, 6, 12, 7, 11, 10]
    assert torch.equal(tpl.rows(test, perm), whole[perm])
    with pytest.raises(ValueError, match="L_out"):
        tpl.rows(_record(T=90, L_out=3), [0])
    with pytest.raises(IndexError):
        tpl.dates(test, test.num_samples)


def test_schaake_template_over_a_materialised_target_and_rows_without_a_slot():
    """A dataset with Y (T, H, W, L_out) instead of the series: the series is rebuilt, its row 0 (NaN: in no window's target)
    is never a date; rows past the time features (the tail of the rebuilt series) are no candidates while slots are in use."""
    from tecmollm.coherence import SchaakeTemplate
    train = _record(T=200, series=False, seed=4)
    tpl = SchaakeTemplate(train, 6, same_slot=False, min_gap=1)
    assert tpl.series.shape == (204, 5) and tpl.first_row == 1 and torch.isnan(tpl.series[0]).all()
    assert torch.equal(tpl.series[1:201], train.Y[:, 0, :, 0]) and torch.equal(tpl.series[201:], train.Y[-1, 0, :, 1:].t())
    seen = np.concatenate([tpl.dates(train, i) for i in range(60)])
    assert seen.min() >= 1 and seen.max() <= 200 and seen.max() > 190
    slotted = SchaakeTemplate(train, 6, min_gap=1)
    seen = np.concatenate([slotted.dates(train, i) for i in range(60)])
    assert seen.min() >= 1 and seen.max() <= 199                        # row 200 and later carry no time feature


def test_schaake_template_raises_when_too_few_dates_qualify():
    from tecmollm.coherence import SchaakeTemplate
    train = _record(T=100, seed=1)
    SchaakeTemplate(train, 8).rows(train, [0])                           # 8 of the 8 or 9 rows per slot
    with pytest.raises(ValueError, match="candidate dates"):
        SchaakeTemplate(train, 10).rows(train, [0])                      # a slot has at most 9 rows
    with pytest.raises(ValueError, match="candidate dates"):
        SchaakeTemplate(train, 8, same_slot=False, min_gap=20).rows(train, [0])   # 97 rows hold at most 5 dates 20 apart
    for bad in (dict(k=1), dict(k=65), dict(k=4, min_gap=0)):
        with pytest.raises(ValueError):
            SchaakeTemplate(train, **bad)


# ------------------------------------------------------------------------------------ members of a quantile forecast
@pytest.mark.parametrize("taus, K", [((0.05, 0.25, 0.5, 0.75, 0.95), 16), ((0.1, 0.5, 0.9), 8), ((0.5,), 4),
                                     ((0.05, 0.25, 0.5, 0.75, 0.95), 3), ((0.02, 0.5, 0.98), 64), ((0.25, 0.5), 2)])
def test_quantile_members_equal_the_restatement(taus, K):
    from tecmollm.coherence import quantile_members
    rng = np.random.default_rng(len(taus) * 100 + K)
    lv = np.sort(rng.standard_normal((3, len(taus), 2, 11)).astype(np.float32), axis=1)
    lv[0, :, 0, :3] = lv[0, ::-1, 0, :3]                                 # crossing levels: sorted before use
    lv[1, 0, 1, 4] = np.nan
    got = quantile_members(torch.from_numpy(lv.copy()), taus, K)
    assert got.dtype == torch.float32 and got.shape == (K, 3, 2, 11)
    want = CR.quantile_members(lv, taus, K)
    assert np.array_equal(got.numpy(), want, equal_nan=True)
    ok = np.isfinite(want).all(axis=0)
    assert (np.diff(want, axis=0)[:, ok] >= 0).all()                     # the comonotone ensemble: members ascend with k
    z = np.sort(lv, axis=1)
    assert (want[:, ok] >= z[:, 0][ok]).all() and (want[:, ok] <= z[:, -1][ok]).all()    # no tail is invented
    with pytest.raises(ValueError):
        quantile_members(torch.from_numpy(lv[:, :1]), (0.1, 0.9), 4)
    with pytest.raises(ValueError):
        quantile_members(torch.from_numpy(lv), taus, 0)


# ------------------------------------------------------------------------------------ the binding
def test_binding_exports_the_reorder_and_python_refuses_host_tensors():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    import ctypes
    import tecmollm
    from tecmollm import _lib
    assert "tecm_member_reorder" in _lib.EXPORTS and hasattr(ctypes.CDLL(LIB), "tecm_member_reorder")
    assert ctypes.sizeof(_lib.TecmMemberReorder) == 23 * 8
    for name in ("reorder_members", "SchaakeTemplate", "EccTemplate", "quantile_members", "evaluate_quantile_ensemble"):
        assert getattr(tecmollm, name) is getattr(tecmollm.coherence, name)
    v = torch.zeros(4, 2, 3, 5)
    with pytest.raises(ValueError, match="GPU"):
        tecmollm.reorder_members(v, v.clone())
    with pytest.raises(ValueError, match=r"\[2, 64\]"):
        tecmollm.reorder_members(v[:1], v[:1].clone())
    import inspect
    from src.models.baselines import AnalogBaseline
    assert inspect.signature(tecmollm.evaluate_analog_ensemble).parameters["reorder"].default is None
    assert inspect.signature(AnalogBaseline.members).parameters["reorder"].default is None
