"""Host-side checks of the quantile forecasts (no GPU): the numpy restatement on hand-worked cases, the derived scores, the
layout convention, the wrapper's argument checks, the files and the C ABI."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

from tests import quantile_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------ the restatement by hand
def test_pinball_two_levels_two_samples_by_hand():
    """taus (0.25, 0.75), y = (1, 3); level 0.25 forecasts (2, 2), level 0.75 forecasts (0, 4).
    u = y - p: level 0: (-1, 1) -> rho = (-1)(0.25 - 1), 1 * 0.25 = 0.75, 0.25;  level 1: (1, -1) -> 0.75, (-1)(0.75 - 1) = 0.25.
    level means 0.5 and 0.5, loss 0.5; gradient g ([u < 0] - tau) with g = 1 / 4: level 0: (0.1875, -0.0625), level 1:
    (-0.1875, 0.0625)."""
    pred = np.array([2, 2, 0, 4], np.float32).reshape(1, 2, 1, 2)
    target = np.array([1, 3], np.float32).reshape(1, 1, 2)
    for h_fast in (True, False):
        loss, levels, dpred, mags = QR.pinball(pred, target, (0.25, 0.75), 1.0, h_fast)
        assert loss == np.float32(0.5) and levels.tolist() == [0.5, 0.5] and mags.tolist() == [1.0, 1.0]
        assert dpred.reshape(-1).tolist() == [0.1875, -0.0625, -0.1875, 0.0625]


def test_pinball_on_the_quantile_takes_the_minus_tau_branch():
    pred = np.array([5.0, 5.0], np.float32).reshape(1, 2, 1, 1)
    loss, levels, dpred, _ = QR.pinball(pred, np.array([5.0], np.float32).reshape(1, 1, 1), (0.25, 0.5), 2.0)
    assert loss == 0 and levels.tolist() == [0, 0] and dpred.reshape(-1).tolist() == [-0.25, -0.5]      # g = 2 / 2


def _acc(levels, target, taus, ids=None, G=1, scaler=None, adjust=None):
    S, Q, H, I = np.shape(levels)
    rows = 1 + Q + Q // 2
    st, ct, mg = np.zeros((G, H, rows, I)), np.zeros((G, H, rows, I), np.int64), np.zeros((G, H, rows, I))
    z = QR.accumulate(st, ct, mg, np.asarray(levels, np.float32), np.asarray(target, np.float32), taus, ids, scaler, adjust)
    return st, ct, z


def test_stats_two_levels_two_samples_by_hand():
    """taus (0.25, 0.75); sample 0: levels (1, 3), y = 2 (inside); sample 1: levels (1, 3), y = 5 (above).
    rho_0.25: (2-1) 0.25 = 0.25, (5-1) 0.25 = 1 -> 1.25;  rho_0.75: (2-3)(0.75-1) = 0.25, (5-3) 0.75 = 1.5 -> 1.75;
    hits: y <= z: level 0: none, level 1: sample 0;  pair: width 2 + 2, covered once."""
    lv = np.array([[1, 3], [1, 3]], np.float32).reshape(2, 2, 1, 1)
    st, ct, z = _acc(lv, np.array([2, 5], np.float32).reshape(2, 1, 1), (0.25, 0.75))
    assert st.reshape(-1).tolist() == [2.0, 1.25, 1.75, 4.0] and ct.reshape(-1).tolist() == [0, 0, 1, 1]
    assert z.reshape(-1).tolist() == [1, 3, 1, 3]


def test_stats_a_crossing_pair_is_counted_and_sorted():
    """Levels emitted as (3, 1): a crossing; scored as (1, 3)."""
    st, ct, z = _acc(np.array([3, 1], np.float32).reshape(1, 2, 1, 1), np.array([2], np.float32).reshape(1, 1, 1), (0.25, 0.75))
    assert z.reshape(-1).tolist() == [1, 3] and ct.reshape(-1).tolist() == [1, 0, 1, 1]
    assert st.reshape(-1).tolist() == [1.0, 0.25, 0.25, 2.0]


def test_stats_y_exactly_on_a_quantile():
    """y = z_lo = 1: rho_lo = 0 (the [y < z] indicator is 0), a hit (y <= z), and the pair covers (lo <= y)."""
    st, ct, _ = _acc(np.array([1, 3], np.float32).reshape(1, 2, 1, 1), np.array([1], np.float32).reshape(1, 1, 1), (0.25, 0.75))
    assert st.reshape(-1).tolist() == [1.0, 0.0, 0.5, 2.0] and ct.reshape(-1).tolist() == [0, 1, 1, 1]
    assert QR.cqr_scores(np.array([1, 3], np.float32).reshape(1, 2, 1, 1), np.array([1], np.float32).reshape(1, 1, 1), 0, 1,
                         None).item() == 0.0


def test_stats_groups_adjust_and_the_value_pipeline():
    lv = np.array([[np.nan, 1.0, 2.0], [0.0, np.inf, 1.0]], np.float32).reshape(2, 3, 1, 1)
    y = np.array([1.0, -np.inf], np.float32).reshape(2, 1, 1)
    adj = np.zeros((2, 1, 3, 1), np.float32)
    adj[1, 0, 0], adj[1, 0, 2] = -0.5, 0.5
    st, ct, z = _acc(lv, y, (0.25, 0.5, 0.75), ids=np.array([1, 7]), G=2, scaler=(10.0, 2.0), adjust=adj)
    # sample 0 (group 1): levels -> (0, 1, 2) scaled -> (10, 12, 14), y -> 12; adjust: (9.5, 12, 14.5); sample 1: bad id, skipped
    assert z[0].reshape(-1).tolist() == [9.5, 12.0, 14.5] and st[0].sum() == 0 and ct[0].sum() == 0
    assert st[1].reshape(-1).tolist() == [1.0, 2.5 * 0.25, 0.0, 2.5 * 0.25, 5.0] and ct[1].reshape(-1).tolist() == [0, 0, 1, 1, 1]
    # -inf truth -> 0 TECU; +inf level -> raw 0 -> the mean
    assert QR.values(lv[1:], y[1:], (10.0, 2.0))[0].reshape(-1).tolist() == [10.0, 10.0, 12.0]
    assert QR.values(lv[1:], y[1:], (10.0, 2.0))[1].item() == 0.0


# ------------------------------------------------------------------------------------ derived scores
def test_winkler_identity_and_the_derived_scores():
    """(2 / alpha)(rho_lo + rho_hi) of a symmetric pair is the Winkler score of the interval, sample by sample; and
    `derive_quantiles` turns the sums into the documented means."""
    from src.evaluation.metrics import crps_weights, derive_quantiles, quantile_pairs
    rng = np.random.default_rng(0)
    taus = (0.05, 0.25, 0.5, 0.75, 0.95)
    S = 200
    z = np.sort(rng.standard_normal((S, 5)) * 3, axis=1)
    y = rng.standard_normal(S) * 4
    y[:5] = z[:5, 0]                                                       # on the lower edge
    for r, (lo_t, hi_t, alpha) in enumerate(quantile_pairs(taus)):
        assert (lo_t, hi_t) == (taus[r], taus[4 - r]) and abs(alpha - 2 * lo_t) < 1e-15
        direct = QR.winkler_direct(z[:, r], z[:, 4 - r], y, alpha)
        via = (2 / alpha) * (QR.rho(y, z[:, r], lo_t) + QR.rho(y, z[:, 4 - r], hi_t))
        np.testing.assert_allclose(via, direct, rtol=1e-12, atol=1e-12)
    st, ct, _ = _acc(z.astype(np.float32).reshape(S, 5, 1, 1), y.astype(np.float32).reshape(S, 1, 1), taus)
    d = derive_quantiles(st[0, 0].T, ct[0, 0].T, taus)                     # (I = 1, rows)
    z32, y32 = z.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    t32 = np.asarray(taus, np.float32).astype(np.float64)
    pin = np.array([QR.rho(y32, z32[:, q], t32[q]).mean() for q in range(5)])
    np.testing.assert_allclose(d["pinball"][0], pin, rtol=1e-12)
    assert d["count"][0] == S and d["crossing_rate"][0] == 0
    np.testing.assert_allclose(d["reliability"][0], [(y32 <= z32[:, q]).mean() for q in range(5)])
    np.testing.assert_allclose(d["interval_width"][0], [(z32[:, 4 - r] - z32[:, r]).mean() for r in range(2)], rtol=1e-12)
    np.testing.assert_allclose(d["coverage"][0], [((z32[:, r] <= y32) & (y32 <= z32[:, 4 - r])).mean() for r in range(2)])
    np.testing.assert_allclose(d["interval_score"][0], [(2 / a) * (pin[r] + pin[4 - r]) for r, (_, _, a) in
                                                        enumerate(quantile_pairs(taus))], rtol=1e-12)
    w = crps_weights(taus)
    np.testing.assert_allclose(w, [0.1, 0.225, 0.25, 0.225, 0.1], rtol=1e-12)
    np.testing.assert_allclose(d["quantile_crps"][0], 2 * (w * pin).sum(), rtol=1e-12)
    assert crps_weights((0.5,)).tolist() == [1.0]
    empty = derive_quantiles(np.zeros((2, 8)), np.zeros((2, 8), np.int64), taus)
    assert np.isnan(empty["pinball"]).all() and empty["pinball"].shape == (2, 5) and empty["coverage"].shape == (2, 2)
    assert np.isnan(empty["quantile_crps"]).all() and (empty["count"] == 0).all()


# ------------------------------------------------------------------------------------ the convention and the wrapper
def test_quantile_config_and_the_layout_convention():
    from tecmollm import quantile_config
    from tecmollm.functions import quantile_view
    cfg = {"prediction_horizon": 4, "num_nodes": 12}
    q = quantile_config(cfg, (0.1, 0.5, 0.9))
    assert q == {"prediction_horizon": 12, "num_nodes": 12} and cfg["prediction_horizon"] == 4      # a copy
    B, Q, L, N = 2, 3, 4, 5
    storage = torch.arange(B * N * Q * L, dtype=torch.float32).view(B, N, Q * L)
    out = storage.permute(0, 2, 1).unsqueeze(-1)                           # the model's (B, Q * L, N, 1) view
    v = quantile_view(out, Q)
    assert v.shape == (B, Q, L, N) and v.data_ptr() == out.data_ptr()
    for q_, h in ((0, 0), (1, 3), (2, 1)):
        assert torch.equal(v[:, q_, h], out[:, q_ * L + h, :, 0])          # j = q * L_out + h
    assert v.stride() == (N * Q * L, L, 1, Q * L)
    with pytest.raises(ValueError):
        quantile_view(out, 5)


class _Stub(torch.nn.Module):
    def __init__(self, channels, N=3):
        super().__init__()
        self.channels, self.N = channels, N

    def forward(self, x, tf, ei, ew=None):
        B = x.shape[0]
        return torch.arange(B * self.N * self.channels, dtype=torch.float32).view(B, self.N, self.channels).permute(0, 2, 1).unsqueeze(-1)


def test_quantile_model_checks_its_levels_and_returns_views():
    from tecmollm import PinballLoss, QuantileModel
    for bad, what in (((0.1, 0.9), "0.5"), ((0.5, 0.1, 0.9), "increase"), ((0.1, 0.5, 0.5, 0.9), "increase"),
                      ((0.0, 0.5, 0.9), r"inside \(0, 1\)"), ((0.1, 0.5, 1.0), r"inside \(0, 1\)"),
                      (tuple((i + 1) / 18 for i in range(17)), "between 1 and 16")):
        with pytest.raises(ValueError, match=what):
            QuantileModel(_Stub(3), bad, 1)
    with pytest.raises(ValueError, match="increase"):
        PinballLoss((0.9, 0.1))
    qm = QuantileModel(_Stub(6), (0.1, 0.5, 0.9), 2)
    x = torch.zeros(2, 1)
    med = qm(x, None, None)
    full = qm.model(x, None, None)
    assert torch.equal(qm.quantiles_of(med), qm.quantiles(x, None, None)) and qm.quantiles_of(med).data_ptr() == med.data_ptr() - 8
    with pytest.raises(ValueError, match="slice"):
        qm.quantiles_of(med.clone())
    assert med.shape == (2, 2, 3, 1) and torch.equal(med, full[:, 2:4]) and med._base is not None
    lv = qm.quantiles(x, None, None)
    assert lv.shape == (2, 3, 2, 3) and torch.equal(lv[:, 1], med[..., 0]) and torch.equal(lv[:, 2, 1], full[:, 5, :, 0])
    with pytest.raises(ValueError, match="must return"):
        QuantileModel(_Stub(5), (0.1, 0.5, 0.9), 2)(x, None, None)


def test_train_step_takes_a_loss_argument():
    from tecmollm import PinballLoss
    from tecmollm.train import TrainStep
    lin = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="loss"):
        TrainStep(lin, optimizer="torch", loss="mse")
    ts = TrainStep(lin, optimizer="torch", loss=PinballLoss((0.1, 0.5, 0.9)))
    with pytest.raises(ValueError, match="Huber"):
        ts.step_graphed(None, None, None, None, None)
    assert TrainStep(lin, optimizer="torch").loss == "huber"


# ------------------------------------------------------------------------------------ files
def test_cqr_intervals_save_and_load(tmp_path):
    from tecmollm import CQRIntervals
    off = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    off[1, 0, 0] = np.inf
    iv = CQRIntervals(off, (0.1, 0.9), (0.1, 0.5, 0.9), [7, 2], 21.5, 9.25, True)
    assert abs(iv.alpha - 0.2) < 1e-15 and not iv.finite and iv.num_groups == 2 and iv.scaler == (21.5, 9.25)
    assert (iv.lo_idx, iv.hi_idx) == (0, 2)
    path = iv.save(str(tmp_path / "cqr"))
    assert path.endswith(".npz")
    with np.load(path, allow_pickle=False) as z:                           # numpy arrays only
        assert sorted(z.files) == ["clip", "counts", "mean", "offset", "pair", "scale", "taus"]
    back = CQRIntervals.load(path)
    assert np.array_equal(back.offset, off) and back.pair == (0.1, 0.9) and back.taus == (0.1, 0.5, 0.9)
    assert back.counts.tolist() == [7, 2] and back.scaler == (21.5, 9.25) and back.alpha == iv.alpha
    adj = back.on("cpu")
    assert adj.shape == (2, 3, 3, 4) and torch.equal(adj[:, :, 0], -adj[:, :, 2]) and (adj[:, :, 1] == 0).all()
    assert CQRIntervals(off[:1], (0.1, 0.9), (0.1, 0.5, 0.9), [7]).finite
    with pytest.raises(ValueError, match="pair"):
        CQRIntervals(off, (0.2, 0.9), (0.1, 0.5, 0.9), [7, 2])


def test_write_quantiles_csv_and_npz(tmp_path):
    from src.evaluation.metrics import QUANTILE_KEYS, QuantileMetrics
    from tecmollm import quantile as QT
    taus = (0.1, 0.5, 0.9)
    G, H, N = 2, 3, 6
    qm = QuantileMetrics(H, N, taus, G, None, device="cpu")
    g = torch.Generator().manual_seed(1)
    qm.stats.copy_(torch.rand(qm.stats.shape, generator=g, dtype=torch.float64) * 10)
    qm.stats[:, :, 0] = 5.0
    qm.counts.copy_(torch.randint(0, 6, qm.counts.shape, generator=g, dtype=torch.int32))
    quant = qm.compute()
    assert set(quant) == set(QUANTILE_KEYS) | {"taus", "pairs", "by_group"}
    assert quant["pinball"].shape == (G, H, N, 3) and quant["coverage"].shape == (G, H, N, 1) and quant["pairs"] == [[0.1, 0.9, 0.1 + 1.0 - 0.9]]
    paths = QT.write_quantiles(quant, str(tmp_path / "out"), grid=(2, 3))
    z = np.load(paths["npz"])
    assert sorted(z.files) == sorted(QUANTILE_KEYS + ("taus", "pairs"))
    assert z["pinball"].shape == (G, H, 2, 3, 3) and z["crossing_rate"].shape == (G, H, 2, 3) and z["taus"].tolist() == list(taus)
    with open(paths["csv"], encoding="utf-8") as f:
        lines = f.read().splitlines()
    cols = QT.quantile_csv_columns(taus)
    assert cols == ["count", "crossing_rate", "quantile_crps", "pinball_0.1", "pinball_0.5", "pinball_0.9", "reliability_0.1",
                    "reliability_0.5", "reliability_0.9", "interval_width_0.1_0.9", "coverage_0.1_0.9", "interval_score_0.1_0.9"]
    assert lines[0] == "group,horizon," + ",".join(cols) and len(lines) == 1 + G * H
    first = lines[1].split(",")
    assert first[:3] == ["0", "0", repr(5.0 * N)]
    # pooled over the nodes: sum of sums / sum of counts
    assert float(first[5]) == pytest.approx(float(qm.stats[0, 0, 1].sum() / (5.0 * N)), rel=1e-14)
    with pytest.raises(ValueError):
        QT.write_quantiles(quant, str(tmp_path / "out"), grid=(2, 2))


# ------------------------------------------------------------------------------------ the C ABI and the build
def test_abi_struct_sizes_and_exports():
    from tecmollm import _lib
    assert _lib.ABI_VERSION == 21 and _lib.TECM_QUANT_MAX_Q == 16 and _lib.TECM_PINBALL_BLOCK_CAP == QR.BLOCK_CAP
    assert ctypes.sizeof(_lib.TecmPinball) == 8 * 5 + 8 * 4 + 4 * 4 + 4 * 16 + 4 + 4 + 8 * 4
    assert ctypes.sizeof(_lib.TecmQuantileStats) == 8 * 5 + 8 * 4 + 8 + 4 + 4 + 8 + 4 + 4 + 4 * 16 + 16 + 16 + 8 * 5 + 8 * 5
    assert ctypes.sizeof(_lib.TecmQuantileScores) == 8 * 5 + 8 * 4 + 8 + 4 + 4 + 8 + 4 + 4 + 16 + 16 + 8 * 3
    assert _lib.TecmPinball.taus.offset == 88 and _lib.TecmQuantileStats.taus.offset == 104
    for name in ("tecm_pinball_fwd_bwd_strided", "tecm_quantile_stats", "tecm_quantile_scores"):
        assert name in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "tecmollm.h"), encoding="utf-8").read()
    assert "#define TECM_QUANT_MAX_Q 16" in header and "#define TECM_ABI_VERSION 21" in header
    for name in ("TecmPinball", "TecmQuantileStats", "TecmQuantileScores"):
        assert f"}} {name};" in header


def test_spill_ceilings_cover_the_quantile_kernels():
    import __graft_entry__ as G
    assert "quantile.hip" in G.SOURCES
    rules = G.SPILL_CEILINGS["quantile.hip"]
    frags = {f for f, _, _ in rules}
    assert {"pinball_stage1_kernel", "pinball_stage2_kernel"} <= frags
    for k in ("stats", "scores"):
        for qp in (1, 2, 4, 8, 16):
            assert f"quantile_{k}_kernelILi{qp}E" in frags
    assert all(field == "ScratchSize [bytes/lane]" and ceiling == 0 for _, field, ceiling in rules)
