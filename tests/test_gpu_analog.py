"""GPU tests of AnalogBaseline: the fused distance sweep and selection (tecm_analog_search) and the gather and mean
(tecm_analog_forecast) against the float64 numpy restatement of tests/analog_ref.py, and the baseline inside tecmollm.evaluate.

Bars.  Integer-valued series in [-8, 8]: every difference, square (<= 256) and sum of up to 512 of them stays below 2^24, so
the distances are exact in fp32 under any order or contraction and indices, distances and counts must EQUAL the restatement's.
Real-valued series: rounding of the difference, of the square and of m additions of non-negative terms gives at most
(m + 3) 2^-24 relative; the bar is twice that, rtol = (m + 4) 2^-23, on every returned distance against the float64 distance
of its own index and against the float64 order statistic of the same rank.  Members: the bits of the gather.  Mean: one fp64
sum rounded once, inside (K + 2) 2^-23 max|member| of the float64 mean."""
import numpy as np
import pytest
import torch

from tests import analog_ref as AR
from tests import linear_ref as LR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def geometry(m=48, K=16, L_out=12):
    """(candidates per staged chunk, queries per block) the host reports."""
    from src.models.baselines import analog_search_geometry
    chunk, tile, _ = analog_search_geometry(3000, 3000 + L_out, max(m, 48) + 20, 7, 2, 1, max(m, 48), L_out, m, K, 3)
    return chunk, tile


def device_search(dev, A, Ty, Xq, starts, L_in, L_out, m, K, key_arch=None, key_q=None, exclude=0, origin_shift=0):
    """A (Ta, N) and Xq (Tq, N) time-major numpy -> numpy (idx, dist, count).  The query series travels as channel 1 of a
    two-channel tensor whose channel 0 is junk, the archive node-major."""
    from src.models.baselines import analog_search
    Ad = torch.tensor(np.ascontiguousarray(A.T)).to(dev)
    X3 = np.stack([np.full_like(Xq, 1e30), Xq], axis=2)
    Xd = torch.tensor(X3).to(dev)
    ka = None if key_arch is None else torch.tensor(np.asarray(key_arch, dtype=np.int32)).to(dev)
    kq = None if key_q is None else torch.tensor(np.asarray(key_q, dtype=np.int32)).to(dev)
    idx, dist, count = analog_search(Ad, Ty, Xd, list(starts), L_in, L_out, m, K, 1, ka, kq, exclude, origin_shift)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy(), count.cpu().numpy()


def assert_equal(got, want, what):
    for g, w, name in zip(got, want, ("idx", "dist", "count")):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g.astype(np.float64), w.astype(np.float64)), (what, name, int((g.astype(np.float64) != w.astype(np.float64)).sum()))


def exact_case(dev, N, S, K, m, ncand, seed, bound=8, L_out=3, ty_equals_ta=False, table=False, **admission):
    """An integer-valued archive with `ncand` candidates and S queries from a series of their own; device against restatement.
    With `table` also the restatement's masked distance table (S, ncand, N)."""
    Ta = max(ncand + m - 1, 1) + (L_out if ty_equals_ta else 0)
    Ty = Ta if ty_equals_ta else Ta + L_out
    L_in = m + 2
    A = AR.integer_series(Ta, N, seed, bound)
    Xq = AR.integer_series(L_in + 2 * S + 1, N, seed + 1, bound)
    starts = (np.arange(S) * 2 + 1)[::-1].copy()                           # descending, odd: the order of the windows is free
    segs = AR.segments(Xq, starts, L_in, m)
    assert AR.n_candidates(Ta, Ty, m, L_out) == max(ncand, 0)
    want = AR.search(A, Ty, segs, K, L_out, admission.get("key_arch"), admission.get("key_q"), admission.get("exclude", 0),
                     None if "exclude" not in admission else starts + L_in + admission.get("origin_shift", 0), want_all=True)
    got = device_search(dev, A, Ty, Xq, starts, L_in, L_out, m, K, **admission)
    assert_equal(got, want[:3], (N, S, K, m, ncand))
    return got + (want[3],) if table else got


# ------------------------------------------------------------------------------------ 1. exact selection
def test_exact_selection_either_side_of_a_chunk_and_across_three(dev):
    """m = 6, K = 5, 7 nodes, 3 queries (one block per node, a tile with one idle query slot): chunk - 1, chunk, chunk + 1 and
    three chunks + 5 candidates, the last also with the outcome series as short as the archive (Ty = Ta bounds the candidates)."""
    chunk, tile = geometry()
    assert 3 * chunk + 5 + 512 <= 3000, "the cases below assume three chunks fit the size cap of this file"
    for ncand in (chunk - 1, chunk, chunk + 1, 3 * chunk + 5):
        exact_case(dev, 7, 3, 5, 6, ncand, 100 + ncand)
    exact_case(dev, 7, 3, 5, 6, 3 * chunk + 5, 7, ty_equals_ta=True)


@pytest.mark.parametrize("N, S, K, m, chunks, extra", [
    (1, 1, 1, 1, 1, 1),            # one node, one query, the nearest alone, a one-step match
    (65, 17, 32, 48, 3, 5),        # the default match length, more than one query tile with a ragged last one, K at its limit
    (7, 3, 32, 512, 1, 1),         # m at its limit: the halo is two thirds of a chunk
    (1, 17, 5, 512, 3, 5),
    (65, 1, 1, 6, 1, -1),
    (7, 17, 5, 1, 1, 0),
])
def test_exact_selection_shapes(dev, N, S, K, m, chunks, extra):
    chunk, _ = geometry()
    got = exact_case(dev, N, S, K, m, chunks * chunk + extra, 11 * N + S + K + m)
    assert (got[2] == K).all()


@pytest.mark.parametrize("ncand, K", [(20, 32), (3, 5), (1, 1), (0, 5), (-7, 5)])
def test_exact_selection_with_fewer_candidates_than_k(dev, ncand, K):
    """Fewer candidates than K, one candidate, none (Ta = m - 1) and an archive far shorter than m: count = the candidates,
    the other places -1 / +inf."""
    idx, dist, count = exact_case(dev, 7, 3, K, 6, ncand, 31 + K)
    assert (count == min(max(ncand, 0), K)).all()
    assert (idx[:, :, max(ncand, 0):] == -1).all() and np.isinf(dist[:, :, max(ncand, 0):]).all()


@pytest.mark.parametrize("K", [5, 32])
def test_exact_selection_with_ties_astride_the_kth_place(dev, K):
    """Values in [-2, 2] and m = 3: a distance takes few values, so the K-th place is tied in most cells and the earlier row
    must win there."""
    chunk, _ = geometry()
    idx, dist, count, want_all = exact_case(dev, 65, 17, K, 3, chunk + 1, 5, bound=2, table=True)
    tied = (want_all == dist[:, None, :, K - 1].astype(np.float64)).sum(axis=1) > (dist == dist[:, :, K - 1:K]).sum(axis=2)
    assert tied.mean() > 0.5, tied.mean()                                   # more rows share the K-th distance than were returned


# ------------------------------------------------------------------------------------ 2. admission
def test_admission_slot_keys_conditions_exclusion_and_both(dev):
    chunk, _ = geometry()
    N, S, K, m, L_out = 7, 17, 5, 6, 3
    ncand = chunk + 40
    Ta = ncand + m - 1
    slot = (np.arange(Ta + 1) % 12).astype(np.int32)
    L_in = m + 2
    starts = (np.arange(S) * 2 + 1)[::-1]
    key_q = ((starts + L_in) % 12).astype(np.int32)
    idx, _, count = exact_case(dev, N, S, K, m, ncand, 3, key_arch=slot, key_q=key_q)
    assert (count == K).all()
    for s in range(S):
        assert ((idx[s] + m) % 12 == key_q[s]).all()
    # a condition with three groups, group 2 absent from the archive: key = 12 * group + slot
    group_arch = (np.arange(Ta + 1) // 100 % 2).astype(np.int32)
    group_q = (np.arange(S) % 3).astype(np.int32)
    idx, dist, count = exact_case(dev, N, S, 32, m, ncand, 3, key_arch=12 * group_arch + slot, key_q=12 * group_q + key_q)
    absent = group_q == 2
    assert (count[absent] == 0).all() and (idx[absent] == -1).all() and np.isinf(dist[absent]).all()
    assert (count[~absent] > 0).all()
    from src.models.baselines import analog_forecast
    mean, members = analog_forecast(torch.zeros(N, Ta + L_out, device=dev), torch.tensor(idx).to(dev), torch.tensor(count).to(dev), m, L_out,
                                    want_members=True)
    gone = torch.tensor(absent).to(dev)
    assert torch.isnan(mean[gone]).all() and torch.isnan(members[:, gone]).all() and not torch.isnan(mean[~gone]).any()


def test_exclusion_with_queries_from_the_archives_own_series(dev):
    """Leave-out evaluation: the queries are windows of the archive itself; without the exclusion every query finds itself at
    distance 0, with exclude = m + L_out no returned origin lies nearer than that, alone and together with slot keys."""
    chunk, _ = geometry()
    N, K, m, L_out, L_in = 7, 5, 6, 3, 8
    Ta = chunk + 60
    A = AR.integer_series(Ta, N, 17)
    Ty = Ta + L_out
    starts = np.array([0, 5, chunk - 4, chunk, Ta - L_in, 300, 301, 302, 311])
    segs = AR.segments(A, starts, L_in, m)
    o_q = starts + L_in
    found_self = device_search(dev, A, Ty, A, starts, L_in, L_out, m, K)
    assert (found_self[1][:, :, 0] == 0).all() and (found_self[0][:, :, 0] + m <= o_q[:, None]).all()
    slot = (np.arange(Ta + 1) % 12).astype(np.int32)
    for keys in (dict(), dict(key_arch=slot, key_q=(o_q % 12).astype(np.int32))):
        exclude = m + L_out
        got = device_search(dev, A, Ty, A, starts, L_in, L_out, m, K, exclude=exclude, **keys)
        assert_equal(got, AR.search(A, Ty, segs, K, L_out, exclude=exclude, o_q=o_q, **keys), ("exclusion", bool(keys)))
        assert (got[2] == K).all() and (np.abs(got[0] + m - o_q[:, None, None]) >= exclude).all()
        # the origin shift: the same archive, numbered from row 40 of a longer series
        shifted = device_search(dev, A, Ty, np.concatenate([AR.integer_series(40, N, 1), A]), starts + 40, L_in, L_out, m, K,
                                exclude=exclude, origin_shift=-40, **keys)
        assert_equal(shifted, got, "origin shift")


# ------------------------------------------------------------------------------------ 3. real-valued inputs
@pytest.mark.parametrize("m, keyed", [(5, False), (48, True), (64, False), (1, False)])
def test_real_valued_distances_and_order_statistics(dev, m, keyed):
    N, S, K, L_out, L_in = 7, 5, 16, 12, max(m, 48)
    Ta = 2000
    A = LR.synthetic(Ta, N, 41, seasonal=True)
    Xq = LR.synthetic(L_in + 40, N, 42, seasonal=True)
    starts = np.array([0, 7, 13, 26, 39])
    segs = AR.segments(Xq, starts, L_in, m)
    keys = dict(key_arch=(np.arange(Ta + 1) % 12).astype(np.int32), key_q=((starts + L_in) % 12).astype(np.int32)) if keyed else {}
    idx, dist, count = device_search(dev, A, Ta + L_out, Xq, starts, L_in, L_out, m, K, **keys)
    _, want_dist, want_count, table = AR.search(A, Ta + L_out, segs, K, L_out, want_all=True, **keys)
    rtol = (m + 4) * 2.0 ** -23
    assert np.array_equal(count, want_count) and (count == K).all()
    worst_own = worst_rank = 0.0
    for s in range(S):
        for n in range(N):
            c, d = idx[s, n].astype(np.int64), dist[s, n].astype(np.float64)
            assert len(set(c.tolist())) == K and (c >= 0).all() and np.isfinite(table[s, c, n]).all()          # (a) admitted, unique
            assert all((d[k], c[k]) < (d[k + 1], c[k + 1]) for k in range(K - 1))                              # (b) ascending by (dist, idx)
            own = np.abs(d - table[s, c, n]) / table[s, c, n]                                                  # (c) its own index's distance
            rank = np.abs(d - want_dist[s, n]) / want_dist[s, n]                                               # (d) the order statistic
            worst_own, worst_rank = max(worst_own, own.max()), max(worst_rank, rank.max())
    print(m, keyed, "worst own / rtol", worst_own / rtol, "worst rank / rtol", worst_rank / rtol)
    assert worst_own <= rtol and worst_rank <= rtol


# ------------------------------------------------------------------------------------ 4. NaN
def test_a_nan_in_the_archive_or_in_a_query_stays_where_it_is(dev):
    chunk, _ = geometry()
    N, S, K, m, L_out, L_in = 7, 3, 5, 6, 3, 8
    Ta = chunk + 50
    A = AR.integer_series(Ta, N, 23)
    Xq = AR.integer_series(3 * L_in, N, 24)
    starts = np.array([0, L_in, 2 * L_in])                                  # the segments do not overlap
    clean = device_search(dev, A, Ta + L_out, Xq, starts, L_in, L_out, m, K)
    # one archive row of node 4: that node never selects a segment that touches it; the other nodes keep their bits
    dirty = A.copy()
    row = int(clean[0][1, 4, 0]) + 2                                        # inside the best match of query 1
    dirty[row, 4] = np.nan
    got = device_search(dev, dirty, Ta + L_out, Xq, starts, L_in, L_out, m, K)
    keep = [n for n in range(N) if n != 4]
    for g, c in zip(got, clean):
        assert np.array_equal(g[:, keep], c[:, keep])
    assert not ((got[0][:, 4] <= row) & (row < got[0][:, 4] + m)).any() and (got[2][:, 4] == K).all()
    assert_equal(got, AR.search(dirty, Ta + L_out, AR.segments(Xq, starts, L_in, m), K, L_out), "NaN in the archive")
    assert not np.array_equal(got[0][1, 4], clean[0][1, 4])
    # one value of the segment of (query 1, node 2): that cell selects nothing, every other cell keeps its bits
    dirty_q = Xq.copy()
    dirty_q[L_in + L_in - 1, 2] = np.nan
    idx, dist, count = device_search(dev, A, Ta + L_out, dirty_q, starts, L_in, L_out, m, K)
    assert count[1, 2] == 0 and (idx[1, 2] == -1).all() and np.isinf(dist[1, 2]).all()
    mask = np.ones((S, N), dtype=bool)
    mask[1, 2] = False
    for g, c in zip((idx, dist, count), clean):
        assert np.array_equal(g[mask], c[mask])
    # a NaN outside the last m steps of the window is not part of the segment
    outside = Xq.copy()
    outside[L_in + L_in - m - 1, 2] = np.nan
    for g, c in zip(device_search(dev, A, Ta + L_out, outside, starts, L_in, L_out, m, K), clean):
        assert np.array_equal(g, c)


# ------------------------------------------------------------------------------------ 5. forecast kernel
@pytest.mark.parametrize("L_out", [1, 12, 13, 32])
def test_forecast_members_are_the_gather_and_the_mean_is_within_its_bound(dev, L_out):
    from src.models.baselines import analog_forecast
    N, B, K, m, Ty = 65, 5, 16, 6, 700
    rng = np.random.default_rng(L_out)
    Y = LR.synthetic(Ty, N, 50 + L_out, seasonal=True)
    ncand = Ty - L_out - m + 1
    idx = rng.integers(0, ncand, (B, N, K)).astype(np.int32)
    idx[0, 0, 0], idx[0, 0, 1] = ncand - 1, 0                               # the last outcome row of the series, and the first
    count = rng.integers(0, K + 1, (B, N)).astype(np.int32)                 # cells with count < K average only their count members
    count[0, 0], count[1, 1], count[2, 2] = K, 0, 1
    idx[np.arange(K)[None, None, :] >= count[:, :, None]] = -1
    want_members, want_mean = AR.forecast(Y, idx, count, m, L_out)
    Yd = torch.tensor(np.ascontiguousarray(Y.T)).to(dev)
    idx_d, count_d = torch.tensor(idx).to(dev), torch.tensor(count).to(dev)
    mean, members = analog_forecast(Yd, idx_d, count_d, m, L_out, want_members=True)
    assert mean.shape == (B, L_out, N) and members.shape == (K, B, L_out, N)
    assert np.array_equal(members.cpu().numpy().astype(np.float64), want_members, equal_nan=True)
    got = mean.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want_mean)) and np.isnan(got[1, :, 1]).all() and not np.isnan(got[2, :, 2]).any()
    bound = (K + 2) * 2.0 ** -23 * np.nanmax(np.abs(want_members))
    err = np.nanmax(np.abs(got - want_mean))
    print(L_out, "mean error / bound", err / bound)
    assert err <= bound
    # the mean alone, into a strided and a permuted output: the same bits, nothing else written
    only, none = analog_forecast(Yd, idx_d, count_d, m, L_out)
    assert none is None and torch.equal(only.nan_to_num(7.0), mean.nan_to_num(7.0))
    wide = torch.full((B, L_out, 2 * N), -7.0, device=dev)
    analog_forecast(Yd, idx_d, count_d, m, L_out, out=wide[:, :, ::2])
    perm = torch.empty(N, B, L_out, device=dev)
    analog_forecast(Yd, idx_d, count_d, m, L_out, out=perm.permute(1, 2, 0))
    assert torch.equal(wide[:, :, ::2].nan_to_num(7.0), mean.nan_to_num(7.0)) and (wide[:, :, 1::2] == -7.0).all()
    assert torch.equal(perm.permute(1, 2, 0).nan_to_num(7.0), mean.nan_to_num(7.0))
    # a NaN outcome propagates to the mean of its cell
    Yn = Y.copy()
    Yn[int(idx[0, 0, 0]) + m, 0] = np.nan
    dirty = analog_forecast(torch.tensor(np.ascontiguousarray(Yn.T)).to(dev), idx_d, count_d, m, L_out)[0]
    assert torch.isnan(dirty[0, 0, 0])


# ------------------------------------------------------------------------------------ 6. reproducibility
def test_two_runs_give_equal_bits_and_the_batching_does_not_matter(dev):
    N, S, K, m, L_out, L_in = 65, 17, 16, 48, 12, 48
    A = LR.synthetic(2500, N, 61, seasonal=True)
    Xq = LR.synthetic(L_in + S, N, 62, seasonal=True)
    starts = np.arange(S)
    slot = (np.arange(2501) % 12).astype(np.int32)
    for keys in (dict(), dict(key_arch=slot, key_q=((starts + L_in) % 12).astype(np.int32))):
        one = device_search(dev, A, 2500 + L_out, Xq, starts, L_in, L_out, m, K, **keys)
        again = device_search(dev, A, 2500 + L_out, Xq, starts, L_in, L_out, m, K, **keys)
        head = device_search(dev, A, 2500 + L_out, Xq, starts[:1], L_in, L_out, m, K,
                             **{k: (v[:1] if k == "key_q" else v) for k, v in keys.items()})
        tail = device_search(dev, A, 2500 + L_out, Xq, starts[1:], L_in, L_out, m, K,
                             **{k: (v[1:] if k == "key_q" else v) for k, v in keys.items()})
        for a, b, h, t in zip(one, again, head, tail):
            assert a.tobytes() == b.tobytes()
            assert a.tobytes() == np.concatenate([h, t]).tobytes()


# ------------------------------------------------------------------------------------ worlds of datasets
L_IN, L_OUT, T_ALL = 48, 12, 600


def make_dataset(dev, y, rows=slice(None), mode="test"):
    """A SeriesWindowDataset (every window) over rows `rows` of a (T, 12) series that is both channel 0 of X and the target;
    the slot column of the time features is the row number mod 12."""
    from src.data.dataset import SeriesWindowDataset
    T = y.shape[0]
    rng = np.random.default_rng(21)
    X = rng.standard_normal((T, 3, 4, 6)).astype(np.float32)
    X[:, :, :, 0] = y.reshape(T, 3, 4)
    TF = np.stack([np.arange(T) % 12, rng.integers(0, 366, T), rng.integers(0, 13, T), rng.integers(0, 4, T)], axis=1).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return SeriesWindowDataset.from_series(t(X[rows]), t(y[rows].reshape(-1, 3, 4)), t(TF[rows]), L_IN, L_OUT, device=dev, mode=mode,
                                           windows="all")


# ------------------------------------------------------------------------------------ 7. a noise-free series
def test_a_periodic_series_is_forecast_exactly(dev):
    from src.models.baselines import AnalogBaseline
    base = np.random.default_rng(8).integers(-8, 9, (12, 12)).astype(np.float32)          # [slot, node]
    y = base[np.arange(T_ALL) % 12]
    train, test = make_dataset(dev, y, slice(0, 396), "train"), make_dataset(dev, y, slice(396, None))
    windows = list(range(len(test)))
    truth = test.batch(windows)[2]
    one = AnalogBaseline(k=1, device=dev).fit(train)
    assert one.match_len_ == 48 and one.H_ == L_OUT and one.num_nodes_ == 12 and one.n_candidates_ == 396 - L_OUT - 48 + 1
    idx, dist, count = one.search_windows(test, windows)
    assert (dist == 0).all() and (count == 1).all()
    assert torch.equal(idx[:, :, 0].cpu(), (torch.arange(len(test)) % 12).int()[:, None].expand(-1, 12))     # every slot-mate matches: the earliest wins
    assert torch.equal(one.forecast_windows(test, windows), truth)
    four = AnalogBaseline(k=4, device=dev).fit(train)
    members = four.members(test, windows)
    assert members.shape == (4, len(test), L_OUT, 12)
    for k in range(4):
        assert torch.equal(members[k].unsqueeze(-1), truth)
    assert (four.search_windows(test, windows)[1] == 0).all()
    # without the slot rule a shifted stretch is no match for a generic periodic series either: the same forecast
    assert torch.equal(AnalogBaseline(k=1, same_slot=False, device=dev).fit(train).forecast_windows(test, windows), truth)


# ------------------------------------------------------------------------------------ 8. end to end
KEYS = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg", "mae_by_horizon", "rmse_by_horizon", "r2_by_horizon",
        "pearson_by_horizon")


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.fixture(scope="module")
def world(dev):
    """The seasonal world of tests/test_gpu_linear.py (600 steps, 12 nodes, seed 1) with the slot column set to the row number
    mod 12: `full` holds every window, `test` the last third of them, and the analog archive is the record behind the first two
    thirds -- the recipe tests/analog_ref.py::held_out_scores restates on the CPU."""
    from oracle import ref_cpu as R
    from src.models.baselines import AnalogBaseline
    from tests.parity import build_model
    y = LR.synthetic(T_ALL, 12, 1, seasonal=True)
    full = make_dataset(dev, y)
    S = len(full)
    n_fit = 2 * S // 3
    test = make_dataset(dev, y, slice(n_fit, None))
    assert S == T_ALL - L_IN - L_OUT + 1 and len(test) == S - n_fit
    cfg = R.default_config(L_in=L_IN, L_out=L_OUT, num_nodes=12)
    model = build_model(cfg, R.init_params(cfg, seed=3), dev, "per_timestep").eval()
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev)
    ana = AnalogBaseline(k=16, device=dev).fit(full, range(n_fit))
    return dict(y=y, full=full, test=test, n_fit=n_fit, model=model, ei=ei, scaler=(20.0, 7.0), ana=ana)


def test_fitted_attributes_search_against_the_restatement_and_the_held_out_property(dev, world):
    from tecmollm import evaluate as E
    y, full, test, n_fit, ana = world["y"], world["full"], world["test"], world["n_fit"], world["ana"]
    Ta, Ty = n_fit - 1 + L_IN, n_fit - 1 + L_IN + L_OUT
    assert (ana.n_candidates_, ana.match_len_, ana.H_, ana.num_nodes_, ana.row0_) == (Ta - 48 + 1, 48, L_OUT, 12, 0)
    by_test = ana.search_windows(test, range(len(test)))
    slots = np.arange(T_ALL) % 12
    starts = np.arange(n_fit, len(full))                                    # the windows of `test` as rows of the whole series
    want = AR.search(y[:Ta], Ty, AR.segments(y, starts, L_IN, 48), 16, L_OUT, slots[:Ta + 1].astype(np.int32),
                     slots[starts + L_IN].astype(np.int32))
    idx, dist, count = (t.cpu().numpy() for t in by_test)
    assert np.array_equal(count, want[2]) and (count == 16).all()
    assert (np.abs(dist - want[1]) <= 52 * 2.0 ** -23 * want[1]).all()
    assert ((idx + 48) % 12 == slots[starts + L_IN][:, None, None]).all()
    truth = test.batch(list(range(len(test))))[2].double()
    score = lambda pred: float(((pred.double() - truth) ** 2).mean().sqrt())
    s = {"analog": score(ana.forecast_windows(test, range(len(test)))), "mean": score(E.window_baseline(test, range(len(test)), "mean"))}
    print(s, AR.held_out_scores(y, slots))
    assert s["analog"] < s["mean"]
    # leave-out on the training split itself: the dataset is the one fitted on, so the exclusion applies
    own = ana.search_windows(full, [0, 100, n_fit - 1])
    o_q = np.array([0, 100, n_fit - 1]) + L_IN
    assert (np.abs(own[0].cpu().numpy() + 48 - o_q[:, None, None]) >= 48 + L_OUT).all() and (own[1] > 0).all()
    assert (own[2] == 16).all()
    # predict: the query is the archive's tail
    out = ana.predict([3, 0, 11, 99], 5)
    assert sorted(out) == [0, 3, 11] and all(v.shape == (5,) and v.dtype == np.float64 and np.isfinite(v).all() for v in out.values())
    segs = y[Ta - 48:Ta][None]
    pi, _, pc = AR.search(y[:Ta], Ty, segs, 16, L_OUT, slots[:Ta + 1].astype(np.int32),
                          np.array([Ta % 12], dtype=np.int32), exclude=48 + L_OUT, o_q=[Ta])
    want_mean = AR.forecast(y[:Ty], pi, pc, 48, L_OUT)[1]
    for n, v in out.items():
        assert np.abs(v - want_mean[0, :5, n]).max() <= 18 * 2.0 ** -23 * np.abs(y).max()


def test_analog_is_a_baseline_of_evaluate_split_maps_combination_and_its_own_ensemble(dev, world, tmp_path):
    import tecmollm
    from src.models.baselines import AnalogBaseline, load_baseline, save_baseline
    from tecmollm import evaluate as E
    from tecmollm.combine import fit_combination
    from tecmollm.ensemble import evaluate_ensemble, write_ensemble
    model, ds, ei, scaler, ana, full = world["model"], world["test"], world["ei"], world["scaler"], world["ana"], world["full"]
    with_a = E.evaluate_split(model, ds, ei, 64, scaler=scaler, baselines=("mean", "last", ana))
    without = E.evaluate_split(model, ds, ei, 64, scaler=scaler, baselines=("mean", "last"))
    assert list(with_a) == ["TEC-MoLLM", "HistoricalAverage", "Persistence", "Analog"]
    for name in without:
        _same(with_a[name], without[name])
    assert with_a["Analog"]["rmse_avg"] < with_a["HistoricalAverage"]["rmse_avg"]
    res, maps = E.evaluate_maps(model, ds, ei, 64, scaler=scaler, baselines=("mean", ana))
    assert list(maps) == ["TEC-MoLLM", "HistoricalAverage", "Analog"] and maps["Analog"]["mae"].shape == (1, L_OUT, 12)
    _same(res["Analog"], with_a["Analog"])
    paths = E.write_report(with_a, str(tmp_path))
    assert "Analog:" in open(paths["summary"]).read() and "\nAnalog," in open(paths["csv"]).read()
    comb = fit_combination(model, ds, ei, 64, members=("model", "mean", ana), ridge=0.01)
    assert comb.member_names == ["model", "mean", "Analog"]
    cres = E.evaluate_split(model, ds, ei, 64, scaler=scaler, baselines=(ana, comb))
    assert list(cres) == ["TEC-MoLLM", "Analog", comb.name] and np.isfinite(cres[comb.name]["rmse_avg"])
    _same(cres["Analog"], with_a["Analog"])
    # the K outcomes as an ensemble
    results, amaps, prob = tecmollm.evaluate_analog_ensemble(ana, ds, 64, scaler=scaler, trim=1)
    _, _, model_prob = evaluate_ensemble(model, ds, ei, 64, members=16, seed=3, scaler=scaler, trim=1, baselines=())
    assert list(results) == ["Analog"] == list(amaps) and set(prob) == set(model_prob)
    assert np.asarray(prob["rank_histogram"]).shape == np.asarray(model_prob["rank_histogram"]).shape == (1, L_OUT, 17)
    _same(results["Analog"], with_a["Analog"])
    assert np.isfinite(prob["crps"]).all() and (prob["crps"] > 0).all() and (prob["count"] == len(ds)).all()
    files = write_ensemble(prob, str(tmp_path))
    assert sorted(files) == ["csv", "npz"] and all(open(p, "rb").read(4) for p in files.values())
    # more members than admitted stretches (about 34 rows per slot, fewer than 32 of them valid candidates in places): raises
    many = AnalogBaseline(k=32, device=dev).fit(full, range(world["n_fit"] // 2))
    with pytest.raises(ValueError, match="fewer than k = 32"):
        tecmollm.evaluate_analog_ensemble(many, ds, 64, scaler=scaler)
    with pytest.raises(ValueError, match="must be fitted"):
        E.evaluate_split(model, ds, ei, 64, scaler=scaler, baselines=(AnalogBaseline(device=dev),))
    with pytest.raises(ValueError, match="must be fitted"):
        tecmollm.evaluate_analog_ensemble(AnalogBaseline(device=dev), ds, 64)
    # pickling: numpy only, the device tensors come back on first use with the same bits
    save_baseline(ana, str(tmp_path / "analog.joblib"))
    back = load_baseline(str(tmp_path / "analog.joblib"))
    assert back._A_dev is None and back.archive_.shape == (12, world["n_fit"] - 1 + L_IN) and back.archive_.dtype == np.float32
    assert torch.equal(back.forecast_windows(ds, [0, 5, len(ds) - 1]), ana.forecast_windows(ds, [0, 5, len(ds) - 1]))
    with pytest.raises(IndexError):
        ana.forecast_windows(ds, [len(ds)])


def test_a_condition_restricts_the_analogs_to_its_group(dev, world):
    """Three storm levels by the row number, level 2 only in the held-out rows: per-sample ids mapped to the origin rows."""
    from src.models.baselines import AnalogBaseline
    full, test, n_fit = world["full"], world["test"], world["n_fit"]
    level = lambda origin: np.where(origin >= n_fit + L_IN + 100, 2, origin // 50 % 2).astype(np.int32)
    fit_ids = level(np.arange(len(full)) + L_IN)                             # one id per sample of `full`
    ana = AnalogBaseline(k=4, device=dev).fit(full, range(n_fit), condition=torch.tensor(fit_ids).to(dev))
    q_ids = level(np.arange(len(test)) + n_fit + L_IN)
    idx, dist, count = (t.cpu().numpy() for t in ana.search_windows(test, range(len(test)), condition=q_ids))
    assert (count[q_ids == 2] == 0).all() and (count[q_ids != 2] == 4).all()
    origin = idx + 48
    for g in (0, 1):
        assert (level(origin[q_ids == g]) == g).all()
    assert ((origin % 12) == ((np.arange(len(test)) + n_fit + L_IN) % 12)[:, None, None])[q_ids != 2].all()
    pred = ana.forecast_windows(test, range(len(test)), condition=q_ids)
    gone = torch.tensor(q_ids == 2).to(dev)
    assert torch.isnan(pred[gone]).all() and not torch.isnan(pred[~gone]).any()
    with pytest.raises(ValueError, match="condition"):
        ana.search_windows(test, [0])
    with pytest.raises(ValueError, match="condition"):
        world["ana"].search_windows(test, [0], condition=q_ids)


# ------------------------------------------------------------------------------------ 9. host refusals
def test_host_refusals_reach_python_as_value_errors_naming_the_argument(dev, world):
    from src.models.baselines import AnalogBaseline, analog_forecast, analog_search
    A = torch.zeros(7, 300, device=dev)
    X = torch.zeros(100, 7, 2, device=dev)
    ok = dict(Ty=312, starts=[0, 1], L_in=48, L_out=12, m=48, K=16)
    analog_search(A, Xq=X, **ok)
    with pytest.raises(ValueError, match="archive must be a tensor on the GPU"):
        analog_search(A.cpu(), Xq=X, **ok)
    with pytest.raises(ValueError, match="X must be a tensor on the GPU"):
        analog_search(A, Xq=X.cpu(), **ok)
    with pytest.raises(ValueError, match="archive must be contiguous"):
        analog_search(torch.zeros(300, 7, device=dev).t(), Xq=X, **ok)
    with pytest.raises(ValueError, match="X must be contiguous"):
        analog_search(A, Xq=torch.zeros(100, 7, 4, device=dev)[:, :, ::2], **ok)
    with pytest.raises(ValueError, match="num_nodes"):
        analog_search(A, Xq=torch.zeros(100, 8, 2, device=dev), **ok)
    for change, reason in ((dict(K=33), "K must"), (dict(K=0), "K must"), (dict(m=49), "m > L_in"), (dict(m=0), "m must"),
                           (dict(L_out=33, Ty=400), "L_out must"), (dict(L_in=101), "shorter than L_in"), (dict(exclude=-1), "exclude"),
                           (dict(channel=2), "channel"), (dict(starts=[]), "at least one window")):
        with pytest.raises(ValueError, match=reason):
            analog_search(A, Xq=X, **{**ok, **change})
    from tecmollm._lib import TecmError
    with pytest.raises(TecmError, match="outside"):
        analog_search(A, Xq=X, **{**ok, "starts": [0, 53]})
    keys = torch.zeros(301, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="together"):
        analog_search(A, Xq=X, key_arch=keys, **ok)
    with pytest.raises(ValueError, match="key_q must have shape"):
        analog_search(A, Xq=X, key_arch=keys, key_q=keys[:3], **ok)
    with pytest.raises(ValueError, match="Tk"):
        analog_search(A, Xq=X, key_arch=keys[:300], key_q=keys[:2], **ok)
    with pytest.raises(ValueError, match="key_arch must be torch.int32"):
        analog_search(A, Xq=X, key_arch=keys.long(), key_q=keys[:2], **ok)
    idx, _, count = analog_search(A, Xq=X, **ok)
    with pytest.raises(ValueError, match="outcomes must be a tensor on the GPU"):
        analog_forecast(torch.zeros(7, 312), idx, count, 48, 12)
    with pytest.raises(ValueError, match="count must have shape"):
        analog_forecast(torch.zeros(7, 312, device=dev), idx, count[:1], 48, 12)
    with pytest.raises(ValueError, match="out must have shape"):
        analog_forecast(torch.zeros(7, 312, device=dev), idx, count, 48, 12, out=torch.zeros(2, 11, 7, device=dev))
    # the fitted baseline against another dataset
    from src.data.dataset import SeriesWindowDataset
    other = world["test"]
    with pytest.raises(ValueError, match="L_out"):
        six = SeriesWindowDataset.from_series(other.X.cpu(), other.Ys.cpu(), other.time_features.cpu(), L_IN, 6, device=dev, mode="test",
                                              windows="all")
        world["ana"].forecast_windows(six, [0])
    with pytest.raises(ValueError, match="match_len"):
        AnalogBaseline(match_len=49, device=dev).fit(world["full"])
    with pytest.raises(ValueError, match="channel"):
        AnalogBaseline(channel=6, device=dev).fit(world["full"])
