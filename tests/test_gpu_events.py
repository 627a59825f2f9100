"""GPU tests of event verification: the two kernels (tecm_event_hist, tecm_event_fss) through `EventMetrics` against the
numpy restatement of tests/events_ref.py, their error words, their reproducibility, and `evaluate_events` end to end on the
tiny model of the other evaluation tests.

Everything the device produces is an integer count, so every comparison with the restatement is `np.array_equal`: there is
no tolerance in this file."""
import os
import socket

import numpy as np
import pytest
import torch

from tests import events_ref as ER

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALER = (21.5, 9.25)
KEYS = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg", "mae_by_horizon", "rmse_by_horizon", "r2_by_horizon",
        "pearson_by_horizon")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _inject(a, rng):
    """NaN, +inf, -inf at three distinct places of a float32 array with at least six elements (else none)."""
    flat = a.reshape(-1)
    if flat.size >= 6:
        where = rng.choice(flat.size, size=3, replace=False)
        flat[where[0]], flat[where[1]], flat[where[2]] = np.nan, np.inf, -np.inf
    return a


def _values(rng, *shape):
    return _inject((rng.standard_normal(shape) * 2.5).astype(np.float32), rng)


def _forecast(layout, K, S, H, I, rng, dev):
    """(device view to feed, numpy (K, S, H, I) of what it holds).  K = 1: the four layouts of tests/test_gpu_error_maps.py;
    K > 1: member-major, and member-major storage (K, S, I, H) seen through the permuted view."""
    if K == 1:
        if layout == "model":                      # (B, N, L_out) permuted: stride_h = 1, stride_i = H
            p = _values(rng, S, I, H)
            return torch.from_numpy(p).to(dev).permute(0, 2, 1).unsqueeze(-1), p.transpose(0, 2, 1)[None]
        if layout == "contiguous":
            p = _values(rng, S, H, I)
            return torch.from_numpy(p).to(dev), p[None]
        if layout == "baseline":                   # one value per (window, node), stride_h = 0
            p = _values(rng, S, I)
            return torch.from_numpy(p).to(dev).view(S, 1, I, 1).expand(S, H, I, 1), np.broadcast_to(p[:, None, :], (S, H, I))[None]
        if layout == "strided":                    # every second node of a wider tensor
            p = _values(rng, S, H, 2 * I)
            return torch.from_numpy(p).to(dev)[:, :, ::2], p[:, :, ::2][None]
    elif layout == "member-major":
        p = _values(rng, K, S, H, I)
        return torch.from_numpy(p).to(dev), p
    elif layout == "permuted":
        p = _values(rng, K, S, I, H)
        return torch.from_numpy(p).to(dev).permute(0, 1, 3, 2).unsqueeze(-1), p.transpose(0, 1, 3, 2)
    raise AssertionError((layout, K))


def _truth(layout, S, H, I, rng, dev):
    if layout == "contiguous":                     # the target takes the permuted layout here
        t = _values(rng, S, I, H)
        return torch.from_numpy(t).to(dev).permute(0, 2, 1), np.ascontiguousarray(t.transpose(0, 2, 1))
    t = _values(rng, S, H, I)
    return torch.from_numpy(t).to(dev).unsqueeze(-1), t


def _thresholds(kind, Q, I, n, scaler, pn, tn, rng):
    """An `EventThresholds` of one of the three addressings, directions alternating from `n`.  Without a scaler the values are
    taken from the data, so that values equal to their threshold occur."""
    from tecmollm.events import EventThresholds
    dirs = [1 if (q + n) % 2 == 0 else -1 for q in range(Q)]
    labels = [f"t{q}" for q in range(Q)]
    phys = np.linspace(10.0, 45.0, Q).astype(np.float32) if Q > 1 else np.array([30.0], dtype=np.float32)
    pool = np.concatenate([pn.reshape(-1), tn.reshape(-1)])
    pool = pool[np.isfinite(pool)]
    if kind == "scalar":
        v = phys if scaler is not None else rng.choice(pool, size=Q).astype(np.float32)
        return EventThresholds(v, (1, 0, 0), dirs, labels)
    if kind == "node":
        if scaler is not None:
            v = (phys[:, None] + rng.standard_normal((Q, I)) * 3).astype(np.float32)
        else:                                      # a member's and the truth's own values (NaN and inf among them)
            v = np.stack([(pn[0, 0, 0] if q % 2 == 0 else tn[0, 0]) for q in range(Q)]).astype(np.float32)
        return EventThresholds(v, (I, 0, 1), dirs, labels, 1, I)
    if kind == "table":
        if scaler is not None:
            v = (phys[:, None, None] + rng.standard_normal((Q, 12, I)) * 3).astype(np.float32)
        else:
            v = rng.choice(pool, size=(Q, 12, I)).astype(np.float32)
            v[:, :, :] = np.where(rng.random((Q, 12, I)) < 0.5, v, tn[0, 0][None, None, :])
        return EventThresholds(v, (12 * I, I, 1), dirs, labels, 12, I)
    raise AssertionError(kind)


def _combos(K):
    """K <= 2: the full product of I, H, S, Q, G.  Larger K: every (I, H) with S, Q and G rotating, so that every value of
    each and both counting paths of the kernel (K = 64: Q = 1 counts in LDS, Q = 3 and 8 in global memory) are met."""
    out, n = [], 0
    for I in (1, 63, 64, 65, 135):
        for H in (1, 12, 50):
            if K <= 2:
                for S in (1, 5):
                    for Q in (1, 3, 8):
                        for G in (1, 3):
                            out.append((I, H, S, Q, G, n))
                            n += 1
            else:
                out.append((I, H, (1, 5)[n % 2], (1, 3, 8)[n % 3], (1, 3)[(n // 2) % 2], n))
                n += 1
    return out


@pytest.mark.parametrize("K, layout", [(1, "model"), (1, "contiguous"), (1, "baseline"), (1, "strided"),
                                       (2, "member-major"), (2, "permuted"), (8, "member-major"), (8, "permuted"),
                                       (64, "member-major"), (64, "permuted")])
def test_histograms_equal_the_restatement(dev, K, layout):
    """I over tile edges, H = 1, 12, 50, S = 1 and 5, Q = 1, 3, 8, G = 1 and 3 (ids out of order, group 1 never visited and
    pre-filled with a sentinel), with and without scaler + clip, NaN and both infinities in forecast and truth, thresholds
    as one value each, per node, and as a (Q, 12, N) table with slots, both directions, two consecutive updates.  Without a
    scaler the thresholds are values of the data: ties occur and are no events."""
    from src.evaluation.metrics import EventMetrics
    from tecmollm import _lib, check_device_errors
    rng = np.random.default_rng(1000 * K + sum(map(ord, layout)))
    ties, paths = 0, set()
    for I, H, S, Q, G, n in _combos(K):
        scaler = SCALER if (I + H + S + G + n) % 2 else None
        kind = ("scalar", "node", "table")[n % 3]
        paths.add((K + 1) * 2 * Q <= _lib.TECM_EVENT_LDS_WORDS)
        em = want = th = None
        for update in range(2):
            pd, pn = _forecast(layout, K, S, H, I, rng, dev)
            td, tn = _truth(layout, S, H, I, rng, dev)
            pn = np.ascontiguousarray(pn)
            if em is None:
                th = _thresholds(kind, Q, I, n, scaler, pn, tn, rng)
                em = EventMetrics(H, I, th, G, scaler, K, device=dev)
                want = np.zeros((G, Q, H, K + 1, 2, I), dtype=np.int64)
                if G == 3:
                    sentinel = torch.arange(Q * H * (K + 1) * 2 * I, device=dev, dtype=torch.int32).view(Q, H, K + 1, 2, I) + 7
                    em.hist[1].copy_(sentinel)
            ids = None
            if G == 3:
                ids = np.array([2, 0, 2, 0, 2][:S] if update == 0 else [0, 2, 2, 0, 0][:S], dtype=np.int32)
            elif update == 1:
                ids = np.zeros(S, dtype=np.int32)                          # the same as None
            slots = rng.integers(0, 12, size=(S, H)).astype(np.int32) if kind == "table" else None
            em.update(pd, td, None if ids is None else torch.from_numpy(ids).to(dev),
                      None if slots is None else torch.from_numpy(slots).to(dev))
            t = ER.accumulate_hist(want, pn, tn, th.values, th.strides, th.dirs, ids, scaler, slots, th.num_slots)
            if scaler is None:
                ties += t
        got = em.hist.cpu().numpy().astype(np.int64)
        what = f"{layout} K={K} I={I} H={H} S={S} Q={Q} G={G} {kind} scaler={scaler is not None}"
        if G == 3:
            assert torch.equal(em.hist[1], sentinel), what + ": the never-visited group was touched"
            got[1] = 0
        assert np.array_equal(got, want), what
        assert got[:, :, :, :, 0].sum() == 2 * S * Q * H * I, what          # every (sample, threshold, horizon, node) once
    print(f"K={K} {layout}: {ties} ties, counting paths (LDS?) {sorted(paths)}")
    assert ties >= 1
    assert paths == ({True, False} if K == 64 else {True})
    check_device_errors()                                                  # no id was out of range


def test_every_contingency_class_is_populated(dev):
    """2.5 N(0, 1) through the scaler (21.5, 9.25) against 15 / 30 / 45 TECU at S * H * I = 2025: the restatement alone shows
    every class of every threshold non-empty, so a kernel that never fires cannot pass; the derived scores are finite."""
    from src.evaluation.metrics import EVENT_CATEGORICAL_KEYS, EventMetrics
    from tecmollm.events import EventThresholds
    rng = np.random.default_rng(2025)
    S, H, I = 5, 3, 135
    p = (rng.standard_normal((S, I, H)) * 2.5).astype(np.float32)
    t = (rng.standard_normal((S, H, I)) * 2.5).astype(np.float32)
    th = EventThresholds.absolute([15.0, 30.0, 45.0])
    want = np.zeros((1, 3, H, 2, 2, I), dtype=np.int64)
    ER.accumulate_hist(want, np.ascontiguousarray(p.transpose(0, 2, 1))[None], t, th.values, th.strides, th.dirs, None, SCALER)
    classes = np.array([[int(c[0, q].sum()) for c in ER.contingency(want)] for q in range(3)])
    print("hits / false alarms / misses / correct negatives per threshold:", classes.tolist())
    assert classes.sum(axis=1).tolist() == [S * H * I] * 3 and classes.min() >= 1             # every class non-empty
    em = EventMetrics(H, I, th, 1, SCALER, device=dev)
    em.update(torch.from_numpy(p).to(dev).permute(0, 2, 1).unsqueeze(-1), torch.from_numpy(t).to(dev).unsqueeze(-1))
    assert np.array_equal(em.hist.cpu().numpy(), want)
    out = em.compute()
    assert out["thresholds"] == th.labels and out["members"] == 1
    assert np.array_equal(out["table_all"][0], classes.astype(np.float64))
    for k in EVENT_CATEGORICAL_KEYS:
        assert out[k].shape == (1, 3, H, I) and np.isfinite(out[k + "_pooled"]).all() and np.isfinite(out[k + "_all"]).all(), k
    a, b, c, d = classes[1].astype(np.float64)
    assert out["csi_all"][0, 1] == a / (a + b + c) and out["pod_all"][0, 1] == a / (a + c)


@pytest.mark.parametrize("K", [1, 8])
def test_bad_group_and_slot_ids_are_skipped_and_reported(dev, K):
    """One sample with a group id outside [0, G), and (sample, horizon) pairs with slot ids -1 and 12: none of them appears in
    any cell, every other cell equals the restatement, and check_device_errors() raises TecmError naming the bit.  An error
    flag, not a fault."""
    from src.evaluation.metrics import EventMetrics
    from tecmollm import TecmError, check_device_errors
    check_device_errors()
    rng = np.random.default_rng(12 + K)
    S, H, I, G, Q = 5, 12, 65, 3, 3
    layout = "model" if K == 1 else "member-major"
    for case in ("group", "slot", "both"):
        pd, pn = _forecast(layout, K, S, H, I, rng, dev)
        td, tn = _truth(layout, S, H, I, rng, dev)
        pn = np.ascontiguousarray(pn)
        th = _thresholds("table", Q, I, 0, SCALER, pn, tn, rng)
        ids = np.array([0, 3 if case != "slot" else 1, 1, 2, 0], dtype=np.int32)
        slots = rng.integers(0, 12, size=(S, H)).astype(np.int32)
        skipped = S * H - (H if case != "slot" else 0)
        if case != "group":
            slots[0, 3], slots[4, 11], slots[2, 0] = -1, 12, 1 << 20
            skipped -= 3
        em = EventMetrics(H, I, th, G, SCALER, K, grid=(5, 13) if K == 1 else None, device=dev)
        em.update(pd, td, torch.from_numpy(ids).to(dev), torch.from_numpy(slots).to(dev))
        want = np.zeros((G, Q, H, K + 1, 2, I), dtype=np.int64)
        ER.accumulate_hist(want, pn, tn, th.values, th.strides, th.dirs, ids, SCALER, slots, 12)
        got = em.hist.cpu().numpy()
        assert np.array_equal(got, want), case
        assert got[:, :, :, :, 0].sum() == skipped * Q * I, case           # the skipped pairs are in no cell
        if case != "group":
            assert got[:, :, 3, :, 0].sum() == (S - 1 - (case == "both")) * Q * I
        if K == 1:
            sums = np.zeros((G, Q, H, 4, 3), dtype=np.int64)
            ER.accumulate_fss(sums, pn[0], tn, th.values, th.strides, th.dirs, (1, 3, 5, 9), (5, 13), ids, SCALER, slots, 12)
            assert np.array_equal(em.sums.cpu().numpy(), sums), case
        flags = {"group": "TECM_BAD_GROUP", "slot": "TECM_BAD_SLOT", "both": "TECM_BAD_GROUP, TECM_BAD_SLOT"}[case]
        with pytest.raises(TecmError, match=flags):
            check_device_errors()
        check_device_errors()                                              # reported once, then clear


def _cover(rows, cols):
    return 2 * max(rows, cols) - 1


@pytest.mark.parametrize("rows, cols", [(1, 1), (1, 7), (5, 27), (41, 71)])
def test_fss_sums_equal_the_brute_force_restatement(dev, rows, cols):
    """S = 2, H = 2, widths 1, 3, 5, 9, the smallest that covers the whole grid from every cell (where it is at most 127) and
    127; three thresholds of which one makes every cell an event and one none; G = 3 with the sentinel group; two updates;
    the forecast in the model's permuted layout."""
    from src.evaluation.metrics import EventMetrics
    from tecmollm import check_device_errors
    from tecmollm.events import EventThresholds
    rng = np.random.default_rng(rows * 100 + cols)
    S, H, I, G = 2, 2, rows * cols, 3
    widths = sorted({1, 3, 5, 9, 127} | ({_cover(rows, cols)} if _cover(rows, cols) <= 127 else set()))
    th = EventThresholds(np.array([0.5, -1e30, 1e30], dtype=np.float32), (1, 0, 0), [1, 1, 1], ["mid", "all", "none"])
    em = EventMetrics(H, I, th, G, None, 1, grid=(rows, cols), scales=widths, device=dev)
    sentinel = torch.arange(3 * H * len(widths) * 3, device=dev, dtype=torch.int64).view(3, H, len(widths), 3) + 11
    em.sums[1].copy_(sentinel)
    want = np.zeros((G, 3, H, len(widths), 3), dtype=np.int64)
    for update in range(2):
        pd, pn = _forecast("model", 1, S, H, I, rng, dev)
        td, tn = _truth("model", S, H, I, rng, dev)
        ids = np.array([2, 0] if update == 0 else [0, 0], dtype=np.int32)
        em.update(pd, td, torch.from_numpy(ids).to(dev))
        ER.accumulate_fss(want, np.ascontiguousarray(pn[0]), tn, th.values, th.strides, th.dirs, widths, (rows, cols), ids)
    got = em.sums.cpu().numpy()
    assert torch.equal(em.sums[1], sentinel), "the never-visited group was touched"
    em.sums[1].zero_()
    got[1] = 0
    assert np.array_equal(got, want), (rows, cols, widths)
    # the all-true field: cf = co = the number of cells of the clipped window; the all-false field: nothing
    assert (got[[0, 2], 2] == 0).all() and (got[[0, 2], 1, :, :, 0] == 0).all() and (got[0, 1, :, :, 1] > 0).all()
    if _cover(rows, cols) <= 127:
        w = widths.index(_cover(rows, cols))
        assert got[2, 1, 0, w].tolist() == [0, I * I * I, I * I * I]       # one sample: every window holds all I cells
        assert np.array_equal(got[:, :, :, w], got[:, :, :, -1])           # 127 covers it too
    out = em.compute()
    assert out["scales"] == widths and out["fss"].shape == (G, 3, H, len(widths)) and out["fss_pooled"].shape == (G, 3, len(widths))
    assert (out["fss"][0, 1] == 1.0).all() and np.isnan(out["fss"][0, 2]).all() and np.isnan(out["fss"][1]).all()
    assert np.array_equal(out["fss"][0, 0], ER.fss(want[0, 0]), equal_nan=True)
    assert np.array_equal(out["fss_uniform"], 0.5 + out["base_rate_pooled"] / 2, equal_nan=True)
    check_device_errors()


@pytest.mark.parametrize("rows, cols", [(5, 27), (41, 71)])
def test_fss_of_a_displaced_field_rises_with_the_width(dev, rows, cols):
    """A field of blobs forecast two columns too far east: the double penalty at the grid scale (width 1) fades as the
    neighbourhood grows.  Asserted on the restatement and, being equal, on the device."""
    from src.evaluation.metrics import EventMetrics
    from tecmollm.events import EventThresholds
    rng = np.random.default_rng(cols)
    truth = np.zeros((rows, cols), dtype=np.float32)
    for _ in range(max(2, rows * cols // 150)):
        r, c = int(rng.integers(0, rows - 1)), int(rng.integers(0, cols - 6))
        truth[r:r + 3, c:c + 4] = 1.0
    pred = np.zeros_like(truth)
    pred[:, 2:] = truth[:, :-2]
    I, widths = rows * cols, (1, 3, 5, 9)
    th = EventThresholds.absolute([0.5])
    want = np.zeros((1, 1, 1, 4, 3), dtype=np.int64)
    ER.accumulate_fss(want, pred.reshape(1, 1, I), truth.reshape(1, 1, I), th.values, th.strides, th.dirs, widths, (rows, cols))
    f = ER.fss(want)[0, 0, 0]
    print(f"{rows} x {cols}: FSS by width {f.tolist()}")
    assert f[0] < f[1] < f[2] < f[3] < 1.0
    em = EventMetrics(1, I, th, grid=(rows, cols), scales=widths, device=dev)
    em.update(torch.from_numpy(pred).to(dev).view(1, 1, I), torch.from_numpy(truth).to(dev).view(1, 1, I))
    assert np.array_equal(em.sums.cpu().numpy(), want)
    got = em.compute()["fss"][0, 0, 0]
    assert np.array_equal(got, f) and got[0] < got[1] < got[2] < got[3]


def test_three_launches_of_each_kernel_are_identical(dev):
    """N = 2911 = 41 x 71, H = 12, B = 16, four groups, a slot table: three fresh accumulations of the histogram (K = 1 with
    the FSS, and K = 16) hold the same bits."""
    from src.evaluation.metrics import EventMetrics
    from tecmollm.events import EventThresholds
    rng = np.random.default_rng(0)
    B, H, N = 16, 12, 2911
    clim = 21.5 + 9.25 * rng.standard_normal((N, 12))
    th = EventThresholds.relative(clim, rel=(0.3, -0.3, 0.0, -0.1))
    p = torch.from_numpy(_values(rng, B, N, H)).to(dev).permute(0, 2, 1).unsqueeze(-1)
    m = torch.from_numpy(_values(rng, 16, B, H, N)).to(dev)
    t = torch.from_numpy(_values(rng, B, H, N)).to(dev).unsqueeze(-1)
    ids = torch.from_numpy(((np.arange(B) * 7) % 4).astype(np.int32)).to(dev)
    slots = torch.from_numpy(rng.integers(0, 12, size=(B, H)).astype(np.int32)).to(dev)
    runs = []
    for _ in range(3):
        e1 = EventMetrics(H, N, th, 4, SCALER, 1, grid=(41, 71), device=dev)
        e16 = EventMetrics(H, N, th, 4, SCALER, 16, device=dev)
        for _ in range(2):
            e1.update(p, t, ids, slots)
            e16.update(m, t, ids, slots)
        runs.append((e1.hist.clone(), e1.sums.clone(), e16.hist.clone()))
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r))
    assert int(runs[0][0][:, :, :, :, 0].sum()) == 2 * B * 4 * H * N == int(runs[0][2][:, :, :, :, 0].sum())
    assert int(runs[0][1].sum()) > 0


# ------------------------------------------------------------------------------------ evaluate_events end to end
@pytest.fixture(scope="module")
def split(dev, golden_dir):
    from oracle import ref_cpu as R
    from src.data.dataset import SlidingWindowSamplerDataset
    from tests.parity import build_model
    g = np.load(os.path.join(golden_dir, "evaluate_split.npz"))
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=12)
    model = build_model(cfg, R.init_params(cfg, seed=3), dev, "per_timestep").eval()
    ds = SlidingWindowSamplerDataset.from_tensors(torch.as_tensor(g["X"]), torch.as_tensor(g["Y"]), torch.as_tensor(g["TF"]),
                                                  int(g["L_in"]), int(g["L_out"]), stride=1, device=dev, mode="test")
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev)
    return g, model, ds, ei, (float(g["mean"]), float(g["scale"]))


def _same(a, b):
    """Two result structures hold the same bits (NaN equal to NaN)."""
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and a and isinstance(a[0], dict):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind == "f")


def _thresholds_for(g, ds, scaler):
    """Relative thresholds on a climatology of the split's own truth per (node, slot), so that both phases occur."""
    from tecmollm.events import EventThresholds
    mean, scale = scaler
    Y = np.asarray(g["Y"], dtype=np.float64) * scale + mean                # (T, 3, 4, L_out)
    N = Y.shape[1] * Y.shape[2]
    clim = np.tile(Y[:, :, :, 0].reshape(len(Y), N).mean(axis=0)[:, None], (1, 12))
    clim += np.arange(12)[None, :] * 0.01
    return EventThresholds.relative(clim, rel=(0.02, -0.02))


def test_evaluate_events_end_to_end_on_a_tiny_model(dev, split, tmp_path):
    """12 nodes on a 3 x 4 grid, 24 windows, batch size 5 (a ragged last batch)."""
    from src.evaluation.metrics import EVENT_CATEGORICAL_KEYS, EVENT_PROBABILISTIC_KEYS, EventMetrics
    from tecmollm import ensemble as EN
    from tecmollm import evaluate as E
    from tecmollm import events as EV
    g, model, ds, ei, scaler = split
    S, N, H = len(ds), 12, 12
    assert S % 5 != 0
    th = _thresholds_for(g, ds, scaler)
    groups = E.window_groups_by_slot(ds) % 3
    before_maps = E.evaluate_maps(model, ds, ei, 5, scaler=scaler, baselines=("mean", "last"), groups=groups, num_groups=3)
    before_ens = EN.evaluate_ensemble(model, ds, ei, 5, members=4, seed=3, scaler=scaler, groups=groups, num_groups=3)
    want = E.evaluate_split(model, ds, ei, 5, scaler=scaler, baselines=("mean", "last"))
    kw = dict(scaler=scaler, baselines=("mean", "last"), groups=groups, num_groups=3, grid=(3, 4), scales=(1, 3, 5))
    res, events = EV.evaluate_events(model, ds, ei, 5, th, **kw)
    assert list(res) == list(want) == list(events) == ["TEC-MoLLM", "HistoricalAverage", "Persistence"]
    for name in want:
        assert set(res[name]) == set(want[name]) == set(KEYS)
        for k in KEYS:
            assert res[name][k] == want[name][k], (name, k)                # exactly
    # the K = 1 tables against the restatement applied to the outputs copied to the host
    everything = list(range(S))
    x, tf, y = ds.batch(everything)
    slots = EV.target_slots(ds, everything)
    assert slots.is_cuda and slots.dtype == torch.int32 and slots.shape == (S, H)
    host_slots = np.array([[int(g["TF"][a + ds.L_in + h, 0]) for h in range(H)] for a in ds.sample_indices])
    assert np.array_equal(slots.cpu().numpy(), host_slots)
    ids = groups.cpu().numpy()
    with torch.no_grad():
        forecasts = {"TEC-MoLLM": model(x, tf, ei), "HistoricalAverage": E.baseline_forecast(ds, everything, "mean"),
                     "Persistence": E.baseline_forecast(ds, everything, "last")}
    tn = y.squeeze(-1).cpu().numpy()
    populated = 0
    for name, pred in forecasts.items():
        pn = np.ascontiguousarray(pred.squeeze(-1).cpu().numpy())
        hist = np.zeros((3, 2, H, 2, 2, N), dtype=np.int64)
        ER.accumulate_hist(hist, pn[None], tn, th.values, th.strides, th.dirs, ids, scaler, host_slots, 12)
        table = np.stack(ER.contingency(hist), axis=3).astype(np.float64)
        assert np.array_equal(events[name]["table"], table), name
        assert events[name]["count"].sum() == 2 * S * H * N
        sums = np.zeros((3, 2, H, 3, 3), dtype=np.int64)
        ER.accumulate_fss(sums, pn, tn, th.values, th.strides, th.dirs, (1, 3, 5), (3, 4), ids, scaler, host_slots, 12)
        assert np.array_equal(events[name]["fss"], ER.fss(sums), equal_nan=True), name
        assert events[name]["scales"] == [1, 3, 5] and events[name]["thresholds"] == th.labels
        per_class = table.sum(axis=(0, 2, 4))                              # (Q, 4)
        assert ((per_class[:, 0] + per_class[:, 2]) > 0).all() and ((per_class[:, 1] + per_class[:, 3]) > 0).all()
        populated += int((per_class > 0).sum())
        for k in EVENT_CATEGORICAL_KEYS:
            assert events[name][k].shape == (3, 2, H, N) and events[name][k + "_pooled"].shape == (3, 2, H)
    print(f"populated (threshold, class) entries over the three forecasts: {populated} of 24")
    # members = 4: the ensemble entry
    res4, ev4 = EV.evaluate_events(model, ds, ei, 5, th, members=4, seed=3, **kw)
    assert model.training is False
    assert list(ev4) == ["TEC-MoLLM", "HistoricalAverage", "Persistence", "TEC-MoLLM-MC"] and _same(res4, res)
    assert all(_same(ev4[name], events[name]) for name in events)
    mc = ev4["TEC-MoLLM-MC"]
    assert mc["members"] == 4 and mc["reliability"].shape == (3, 2, H, 5, 2) and mc["roc_curve"].shape == (3, 2, H, 6, 2)
    assert np.array_equal(mc["reliability"][..., 0].sum(axis=3), mc["count"].sum(axis=3))      # sum_j n_j = count
    assert mc["count"].sum() == 2 * S * H * N and mc["fss"].shape == (3, 2, H, 3)
    for k in EVENT_PROBABILISTIC_KEYS:
        assert mc[k].shape == (3, 2, H, N) and mc[k + "_pooled"].shape == (3, 2, H) and mc[k + "_all"].shape == (3, 2)
        assert k not in events["TEC-MoLLM"]
    ok = np.isfinite(mc["brier_pooled"])
    np.testing.assert_allclose(mc["brier_pooled"][ok], (mc["brier_reliability_pooled"] - mc["brier_resolution_pooled"] +
                                                        mc["brier_uncertainty_pooled"])[ok], rtol=0, atol=1e-14)
    again = EV.evaluate_events(model, ds, ei, 5, th, members=4, seed=3, **kw)[1]
    assert _same(again, ev4)                                               # the same seed reproduces
    other = EV.evaluate_events(model, ds, ei, 5, th, members=4, seed=4, **kw)[1]
    assert _same(other["TEC-MoLLM"], ev4["TEC-MoLLM"])
    # two `order=` halves with first_chunk add up to the full pass exactly
    kept = []
    orig = EventMetrics.compute

    def spy(self):
        kept.append((self.hist.clone(), None if self.sums is None else self.sums.clone()))
        return orig(self)
    EventMetrics.compute = spy
    try:
        EV.evaluate_events(model, ds, ei, 5, th, members=4, seed=3, **kw)
        EV.evaluate_events(model, ds, ei, 5, th, members=4, seed=3, order=list(range(10)), first_chunk=0, **kw)
        EV.evaluate_events(model, ds, ei, 5, th, members=4, seed=3, order=list(range(10, S)), first_chunk=2, **kw)
    finally:
        EventMetrics.compute = orig
    assert len(kept) == 15                                                 # 3 passes x (4 forecasts + the members)
    for i in range(5):
        full, a, b = kept[i], kept[5 + i], kept[10 + i]
        assert torch.equal(full[0], a[0] + b[0]), i
        assert (full[1] is None and a[1] is None) or torch.equal(full[1], a[1] + b[1]), i
    # the other passes are what they were
    assert _same(E.evaluate_maps(model, ds, ei, 5, scaler=scaler, baselines=("mean", "last"), groups=groups, num_groups=3), before_maps)
    assert _same(EN.evaluate_ensemble(model, ds, ei, 5, members=4, seed=3, scaler=scaler, groups=groups, num_groups=3), before_ens)
    # the files
    paths = EV.write_events(ev4, str(tmp_path), grid=(3, 4))
    with np.load(paths["npz"]) as z:
        assert z["TEC-MoLLM/csi"].shape == (3, 2, H, 3, 4) and z["TEC-MoLLM/table"].shape == (3, 2, H, 4, 3, 4)
        assert z["TEC-MoLLM-MC/brier"].shape == (3, 2, H, 3, 4) and "TEC-MoLLM/brier" not in z.files
        assert np.array_equal(z["Persistence/pod"].reshape(3, 2, H, N), ev4["Persistence"]["pod"], equal_nan=True)
    rows = open(paths["csv"]).read().strip().split("\n")
    assert len(rows) == 1 + 4 * 3 * 2 * H and rows[0].startswith("forecast,group,threshold,horizon,hits,false_alarms")
    assert rows[0].endswith("fss_1,fss_3,fss_5,fss_uniform")
    rel = open(paths["reliability"]).read().strip().split("\n")
    assert len(rel) == 1 + 3 * 2 * H * 5 and rel[1].startswith("TEC-MoLLM-MC,0,")
    with pytest.raises(ValueError):
        EV.evaluate_events(model, ds, ei, 5, th, groups=groups[:-1], num_groups=3)
    with pytest.raises(ValueError):
        EV.evaluate_events(model, ds, ei, 5, th, members=1)


def test_target_slots_on_a_series_dataset(dev):
    """`SeriesWindowDataset` in both window modes: the slot of target step h of window a is time_features[a + L_in + h, 0]."""
    from src.data.dataset import SeriesWindowDataset
    from tecmollm.events import target_slots
    T, L_in, L_out = 40, 6, 4
    rng = np.random.default_rng(4)
    X = torch.from_numpy(rng.standard_normal((T, 2, 3, 6)).astype(np.float32))
    Ys = torch.from_numpy(rng.standard_normal((T, 2, 3)).astype(np.float32))
    t = torch.arange(T, dtype=torch.float32)
    TF = torch.stack([(t * 5) % 12, t % 366, torch.zeros(T), (t // 30) % 4], 1)
    for windows in ("reference", "all"):
        ds = SeriesWindowDataset.from_series(X, Ys, TF, L_in, L_out, stride=2, device=dev, windows=windows)
        idx = list(range(len(ds)))[::-1]
        got = target_slots(ds, idx)
        assert got.is_cuda and got.dtype == torch.int32 and got.shape == (len(ds), L_out)
        want = [[int(TF[ds.sample_indices[i] + L_in + h, 0]) for h in range(L_out)] for i in idx]
        assert got.tolist() == want, windows
    with pytest.raises(IndexError):
        target_slots(ds, [len(ds)])


# ------------------------------------------------------------------------------------ the rank merge
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_counts(rank):
    g = torch.Generator().manual_seed(50 + rank)
    hist = torch.randint(0, 1 << 20, (2, 3, 4, 5, 2, 6), generator=g, dtype=torch.int32)
    sums = torch.randint(0, 1 << 40, (2, 3, 4, 2, 3), generator=g, dtype=torch.int64)
    return hist, sums


def _merge_worker(rank, port, out_dir):
    import sys
    import torch.distributed as dist
    for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from src.evaluation.metrics import EventMetrics
    from tecmollm.events import EventThresholds
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    try:
        th = EventThresholds.absolute([10.0, 20.0, 30.0])
        prob = EventMetrics(4, 6, th, 2, None, 4, device="cpu")
        prob.hist.copy_(_rank_counts(rank)[0])
        assert prob.merge_() is prob
        hist1, sums = _rank_counts(rank)
        det = EventMetrics(4, 6, th, 2, None, 1, grid=(2, 3), scales=(1, 3), device="cpu")
        det.hist.copy_(hist1[:, :, :, :2])
        det.sums.copy_(sums)
        det.merge_(dist.new_group([0, 1]))
        torch.save({"prob": prob.hist, "det": det.hist, "sums": det.sums}, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_merge_on_two_gloo_ranks_is_the_plain_sum(tmp_path):
    """The counts of two ranks (host tensors: the ranks open no GPU) after `merge_`: the plain integer sum, on both ranks."""
    import torch.multiprocessing as mp
    mp.spawn(_merge_worker, args=(_free_port(), str(tmp_path)), nprocs=2, join=True)
    (h0, s0), (h1, s1) = _rank_counts(0), _rank_counts(1)
    for rank in (0, 1):
        got = torch.load(os.path.join(tmp_path, f"rank{rank}.pt"))
        assert torch.equal(got["prob"], h0 + h1) and got["prob"].dtype == torch.int32
        assert torch.equal(got["det"], (h0 + h1)[:, :, :, :2]) and torch.equal(got["sums"], s0 + s1)
