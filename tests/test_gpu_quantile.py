"""Quantile forecasts on the device (include/tecmollm.h (3k)): the pinball loss pair, `tecm_quantile_stats`, the CQR score and
calibration against the numpy restatement (tests/quantile_ref.py), the pinball training step against the CPU oracle, and the
evaluation end to end on a tiny model.

Bars: integer counts, scores, offsets and gradients are compared exactly.  A float64 sum is compared with the ordered
restatement at 1e-12 x (sum of |terms|), the project's bar for ordered float64 sums.  A float32 loss on dyadic inputs (every
partial sum exact) is within 2 ulps of the exact mean: one division, one rounding."""
from __future__ import annotations

import os
import socket

import numpy as np
import pytest
import torch

from tests import quantile_ref as QR
from tests import reduction_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-12
SCALER = (21.5, 9.25)
DYADIC = {1: (0.5,), 3: (0.125, 0.5, 0.875), 16: tuple((2 * i + 1) / 32 for i in range(16))}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------ pinball
def _head_view(pred, dev):
    """(B, Q, H, N) values -> the same values as the quantile view of the head's (B, N, Q * H) storage on the device."""
    from tecmollm.functions import quantile_view
    B, Q, H, N = pred.shape
    storage = pred.permute(0, 3, 1, 2).reshape(B, N, Q * H).contiguous().to(dev)
    return quantile_view(storage.permute(0, 2, 1).unsqueeze(-1), Q)


def _framed(t, dev):
    """(B, H, N) target as a window of a wider NaN-filled device tensor."""
    B, H, N = t.shape
    wide = torch.full((B, H + 2, N + 3), float("nan"), device=dev)
    wide[:, 1:H + 1, 2:N + 2] = t.to(dev)
    return wide[:, 1:H + 1, 2:N + 2]


def _dyadic_case(shape, seed):
    """pred (B, Q, H, N), target (B, H, N), u = target - pred: multiples of 0.25 (u in [-3, 3], zero included), so u, every
    rho = u (tau - [u < 0]) at dyadic taus (multiples of 2^-7 below 3) and every partial sum of them are exact."""
    B, Q, H, N = shape
    g = rc.gen("pinball", shape, seed)
    u = torch.randint(-12, 13, shape, generator=g).float() * 0.25
    t = torch.randint(-16, 17, (B, H, N), generator=g).float() * 0.25
    return t[:, None] - u, t, u


def _exact_ref(u, taus, gs):
    B, Q, H, N = u.shape
    n = B * Q * H * N
    tau32 = torch.tensor(taus, dtype=torch.float32)
    neg = (u < 0)
    rho = u.double() * (tau32.double().view(1, Q, 1, 1) - neg.double())
    g = np.float32(gs) / np.float32(n)
    dpred = torch.from_numpy(np.asarray(g * (neg.float().numpy() - tau32.view(1, Q, 1, 1).numpy()), dtype=np.float32))
    return rho.sum().item() / n, [rho[:, q].sum().item() / (n // Q) for q in range(Q)], dpred, float(g)


def _check_exact(dev, shape, gs, seed=0):
    from tecmollm import ops
    taus = DYADIC[shape[1]]
    pred_l, t, u = _dyadic_case(shape, seed)
    pred, target = _head_view(pred_l, dev), _framed(t, dev)
    want_loss, want_levels, want_d, g = _exact_ref(u, taus, gs)
    runs = [ops.pinball_fwd_bwd_strided(pred, target, taus, gs) for _ in range(3)]
    loss, dpred, levels = runs[0]
    assert dpred.stride() == pred.stride() and dpred.shape == pred.shape, shape
    assert torch.equal(dpred.cpu(), want_d), shape
    ul = rc.ulps32(loss.item(), want_loss)
    ull = max(rc.ulps32(levels[q].item(), want_levels[q]) for q in range(shape[1]))
    print(f"pinball exact {shape} gs={gs}: loss {ul:.2f} ulp, levels {ull:.2f} ulp")
    assert ul <= 2 and ull <= 2, (shape, ul, ull)
    zero = (u == 0)
    if zero.any():                                                         # u == 0: the -tau branch
        tau_b = torch.tensor(taus, dtype=torch.float32).view(1, -1, 1, 1).expand_as(u)
        assert torch.equal(dpred.cpu()[zero], (-tau_b * g)[zero])
    for other in runs[1:]:
        assert torch.equal(other[0], loss) and torch.equal(other[1], dpred) and torch.equal(other[2], levels), shape
    loss_only = ops.pinball_fwd_bwd_strided(pred, target, taus, gs, want_grad=False)
    assert loss_only[1] is None and torch.equal(loss_only[0], loss)
    return zero.any().item()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 135])
def test_pinball_exact_on_the_heads_permuted_view(dev, N):
    seen_zero = False
    for B in (1, 2):
        for Q in (1, 3, 16):
            for H in (1, 12):
                seen_zero |= _check_exact(dev, (B, Q, H, N), (1.0, 0.125)[(B + H) % 2])
    assert seen_zero or N == 1


@pytest.mark.parametrize("M", [256 * QR.BLOCK_CAP, 256 * QR.BLOCK_CAP + 1])
def test_pinball_exact_either_side_of_the_block_cap(dev, M):
    """A level of 256 x 1024 elements is the last that gives every thread one element; one more and thread 0 of block 0 walks
    a second one."""
    _check_exact(dev, (1, 3, 1, M), 1.0)
    _check_exact(dev, (2, 1, 12, (M + 23) // 24), 4.0)                     # past the cap with B and H in the decode


@pytest.mark.parametrize("shape", [(2, 3, 12, 135), (1, 3, 1, 65), (2, 3, 12, 11000)])
def test_pinball_at_non_dyadic_levels_matches_the_ordered_restatement(dev, shape):
    """taus (0.1, 0.5, 0.9), N(0, 1) operands, both layouts of pred.  The float64 sums are compared at BAR x sum |terms|; the
    outputs are those sums divided and rounded to float32 once, so half a float32 spacing at the value is added (the output
    format's own rounding, which the restatement applies too).  dpred is one float32 product and compared exactly."""
    from tecmollm import ops
    taus = (0.1, 0.5, 0.9)
    B, Q, H, N = shape
    g = rc.gen("pinball-nd", shape)
    pred_l, t = torch.randn(shape, generator=g), torch.randn((B, H, N), generator=g)
    for h_fast in (True, False):
        pred = _head_view(pred_l, dev) if h_fast else pred_l.to(dev)
        loss, dpred, levels = ops.pinball_fwd_bwd_strided(pred, _framed(t, dev), taus, 0.5)
        w_loss, w_levels, w_d, mags = QR.pinball(pred_l.numpy(), t.numpy(), taus, 0.5, h_fast)
        assert np.array_equal(dpred.cpu().numpy(), w_d) and dpred.stride() == pred.stride()
        M = B * H * N
        for got, want, mag, n in [(loss.item(), w_loss, mags.sum(), Q * M)] + [(levels[q].item(), w_levels[q], mags[q], M) for q in range(Q)]:
            err, bar = abs(got - float(want)), BAR * mag / n + 0.5 * float(np.spacing(np.float32(want)))
            print(f"pinball {shape} h_fast={h_fast}: |kernel - restatement| = {err:.3e} (bar {bar:.3e})")
            assert err <= bar, (shape, h_fast, got, want)


def _torch_pinball(out, y, taus):
    Q = len(taus)
    v = out.squeeze(-1).unflatten(1, (Q, out.shape[1] // Q))
    u = y.squeeze(-1)[:, None] - v
    tau = torch.tensor(taus, dtype=u.dtype, device=u.device).view(1, Q, 1, 1)
    return (u * (tau - (u < 0).to(u.dtype))).mean()


def test_pinball_fn_and_loss_match_torch_autograd_on_the_dyadic_inputs(dev):
    from tecmollm import PinballFn, PinballLoss
    taus = DYADIC[3]
    B, Q, H, N = 2, 3, 4, 64                                               # n = 1536 = 3 * 2^9: fl(1 / n) times a dyadic factor
    pred_l, t, _ = _dyadic_case((B, Q, H, N), 5)
    y = t.unsqueeze(-1).to(dev)
    grads, losses = [], []
    for route in ("fn", "module", "torch"):
        storage = pred_l.permute(0, 3, 1, 2).reshape(B, N, Q * H).contiguous().to(dev).requires_grad_(True)
        out = storage.permute(0, 2, 1).unsqueeze(-1)
        loss = {"fn": lambda: PinballFn.apply(out, y, taus), "module": lambda: PinballLoss(taus)(out, y),
                "torch": lambda: _torch_pinball(out, y, taus)}[route]()
        loss.backward()
        grads.append(storage.grad.clone())
        losses.append(loss.item())
    assert torch.equal(grads[0], grads[2]) and torch.equal(grads[1], grads[2])
    assert losses[0] == losses[1] and abs(losses[0] - losses[2]) <= 2 * float(np.spacing(np.float32(losses[2])))


class _Head(torch.nn.Module):
    """x (B, N, F) -> (B, Q * L, N, 1), the permuted view of a (B, N, Q * L) product, as the model's head returns it."""

    def __init__(self, F, QL):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(F, QL, generator=torch.Generator().manual_seed(1)) * 0.25)
        self.douts = []

    def forward(self, x, tf, ei, ew=None):
        out = (x @ self.w).permute(0, 2, 1).unsqueeze(-1)
        if out.requires_grad:
            out.register_hook(lambda g: self.douts.append(g.clone()))
        return out


def test_train_step_hands_autograd_the_dout_of_the_unfused_route(dev):
    from tecmollm import PinballLoss
    from tecmollm.train import TrainStep
    taus = (0.1, 0.5, 0.9)
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(2, 65, 7, generator=g).to(dev), torch.randn(2, 4, 65, 1, generator=g).to(dev)
    got = []
    for fused in (True, False):
        model = _Head(7, 12).to(dev)
        ts = TrainStep(model, accumulation_steps=2, fused_huber=fused, loss=PinballLoss(taus))
        loss = ts.step(x, None, None, None, y)
        got.append((loss.clone(), model.douts[0]))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert got[0][1].abs().max() > 0


# ------------------------------------------------------------------------------------ the whole step
def test_whole_pinball_step_matches_the_cpu_oracle(dev):
    """N = 12 on a 3 x 4 grid, B = 2, L_in = 48, L_out = 4, Q = 3, fp32, training mode with mirrored dropout masks: forward,
    loss and every trainable gradient within `assert_parity`'s standard fp32 bars."""
    from oracle import ref_cpu as R
    from src.model import modules as M_
    from tecmollm import PinballFn
    from tests import parity as P
    taus, L_out, B, seed = (0.1, 0.5, 0.9), 4, 2, 0
    cfg = R.default_config(L_in=48, L_out=len(taus) * L_out, num_nodes=12)
    params = R.init_params(cfg, seed=seed)
    x, tf, y = R.synthetic_batch(B, 48, 12, cfg["spatial_in_channels_base"], L_out, seed=seed + 100)
    ei, ew = R.grid_graph(3, 4, threshold_km=170.0)
    torch.manual_seed(4242 + seed)
    M_._seed_counter[0] = 17
    masks = P.device_masks(cfg, B, ei, torch.initial_seed() + 7919 * 18, "reference")
    p = {k: v.clone().requires_grad_(R.is_trainable(k)) for k, v in params.items()}
    out_ref = R.forward(x, tf, ei, p, cfg, 1, q=R.FP32, masks=masks)
    loss_ref = _torch_pinball(out_ref, y, taus)
    names = [k for k, v in p.items() if v.requires_grad]
    grads = torch.autograd.grad(loss_ref, [p[k] for k in names], allow_unused=True)
    grads_ref = {k: (g if g is not None else torch.zeros_like(p[k])) for k, g in zip(names, grads)}

    model = P.build_model(cfg, params, dev, "reference").train()
    tfd = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(B, 48, 12, 4)
    out = model(x.to(dev), tfd, ei.to(dev), ew.to(dev))
    loss = PinballFn.apply(out, y.to(dev), taus)
    loss.backward()
    torch.cuda.synchronize()
    out_ref = out_ref.detach()
    res = {"fwd_rel": P.rel_err(out, out_ref), "fwd_elem": P.elem_err(out, out_ref), "precision": "fp32",
           "loss_rel": abs(loss.item() - loss_ref.item()) / abs(loss_ref.item())}
    named, per, tight = dict(model.named_parameters()), {}, {}
    worst = worst_e = worst_k = 0.0
    for k, gref in grads_ref.items():
        gd = named[k].grad
        assert gd is not None, k
        nz = gref.abs().max() > 0
        e = P.rel_err(gd, gref) if nz else float(gd.abs().max())
        ee = P.elem_err(gd, gref) if nz else float(gd.abs().max())
        per[k] = (e, ee, P.l2_rel(gd, gref) if nz else 0.0)
        worst = max(worst, e)
        if k in P.KINK_TENSORS:
            worst_k = max(worst_k, P.elem_err(gd, gref, P.RTOL, P.ATOL_RMS_KINK) if nz else float(gd.abs().max()))
            tight[k] = ee
        else:
            worst_e = max(worst_e, ee)
    res.update(grad_rel_max=worst, grad_elem_max=worst_e, kink_elem_max=worst_k, kink_elem_tight=tight, n_grads=len(per),
               per_param=per, frozen_with_grad=[k for k, v in named.items() if not R.is_trainable(k) and v.grad is not None])
    print({k: v for k, v in res.items() if k != "per_param"})
    assert out.shape == (B, 12, 12, 1) and res["n_grads"] > 10
    P.assert_parity(res)


SPATIAL_STAGE = ("spatio_temporal_embedding.", "spatial_encoder.")


def _two_steps(dev, freeze_spatial=False, snaps=None, **kw):
    """Two `TrainStep.step` calls on a 12-node model in training mode from one seed: (flat parameters before, after, losses);
    with `snaps` a list, it receives after every step the trainable parameters outside the spatial stage, concatenated."""
    from oracle import ref_cpu as R
    from src.model import modules as M_
    from tecmollm.train import TrainStep
    from tests import parity as P
    Q = 1 if isinstance(kw.get("loss", "huber"), str) else len(kw["loss"].taus)
    cfg = R.default_config(L_in=16, L_out=4 * Q, num_nodes=12)
    torch.manual_seed(77)
    M_._seed_counter[0] = 0
    model = P.build_model(cfg, R.init_params(cfg, seed=1), dev, "reference").train()
    if freeze_spatial:
        for name, p in model.named_parameters():
            if name.startswith(SPATIAL_STAGE):
                p.requires_grad_(False)
    ts = TrainStep(model, **kw)
    before = ts.optimizer.flat_param.clone()
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev)
    losses = []
    for s in range(2):
        x, tf, y = R.synthetic_batch(2, 16, 12, cfg["spatial_in_channels_base"], 4, seed=200 + s)
        tfd = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(2, 16, 12, 4)
        losses.append(ts.step(x.to(dev), tfd, ei, None, y.to(dev)).item())
        if snaps is not None:
            snaps.append(torch.cat([p.detach().reshape(-1) for name, p in model.named_parameters()
                                    if p.requires_grad and not name.startswith(SPATIAL_STAGE)]).clone())
    return before, ts.optimizer.flat_param.clone(), losses


def test_two_train_steps_with_the_pinball_loss_and_the_untouched_default(dev):
    """The pinball step trains (finite loss, parameters move).  `TrainStep(model)` and `TrainStep(model, loss="huber")` are
    one code path: the flat parameter buffers after two steps are compared bit for bit.  The comparison runs with the eleven
    spatial-stage parameters frozen: their gradients are accumulated with float atomics (csrc/spatial_bwd.hip), whose order
    differs from run to run, so two runs of the SAME default step already differ in the last bit of one or two of 1.85 M
    parameters (measured on the default code path, eight repeats of one construction: seven differ from the first, max
    |diff| 7.5e-9 in at most 2 parameters) -- with them frozen that launch is skipped and the step is a deterministic
    function of its inputs (ten repeats, both constructions: identical bits).  With everything trainable, what does not
    depend on the order of those atomics is compared bit for bit as well: the loss of the first step, and after the first
    step every trainable parameter outside the spatial stage (their gradients do not pass through the tables' sums; the
    clip coefficient, the one thing they share with them, is exactly 1 while the gradient norm is below max_norm, and the
    first AdamW step moves a parameter by lr * g / (|g| + eps), which a last-bit change of g does not alter either)."""
    from tecmollm import PinballLoss
    before, after, losses = _two_steps(dev, loss=PinballLoss((0.1, 0.5, 0.9)))
    assert all(np.isfinite(losses)) and losses[0] > 0 and not torch.equal(before, after) and torch.isfinite(after).all()
    b0, a0, l0 = _two_steps(dev, freeze_spatial=True)
    b1, a1, l1 = _two_steps(dev, freeze_spatial=True, loss="huber")
    assert torch.equal(b0, b1) and torch.equal(a0, a1) and l0 == l1 and not torch.equal(b0, a0)
    s2, s3 = [], []
    _, _, l2 = _two_steps(dev, snaps=s2)
    _, _, l3 = _two_steps(dev, snaps=s3, loss="huber")
    assert l2[0] == l3[0] == l0[0]
    assert s2[0].numel() > 1_000_000 and torch.equal(s2[0], s3[0]) and not torch.equal(s2[0], s2[1])


def test_default_and_huber_train_steps_agree_bit_for_bit_on_a_head_without_atomics(dev):
    """The same comparison on a stand-in model whose backward is one matrix product: nothing but TrainStep's own route (the
    fused Huber pair, the hand-over into the flat gradient, clip + AdamW) runs, with and without gradient accumulation."""
    from tecmollm.train import TrainStep
    g = torch.Generator().manual_seed(6)
    x, y = torch.randn(2, 65, 7, generator=g).to(dev), torch.randn(2, 4, 65, 1, generator=g).to(dev)
    for acc in (1, 2):
        flats = []
        for kw in ({}, {"loss": "huber"}):
            model = _Head(7, 4).to(dev)
            ts = TrainStep(model, accumulation_steps=acc, **kw)
            losses = [ts.step(x, None, None, None, y).item() for _ in range(2 * acc)]
            flats.append((ts.optimizer.flat_param.clone(), losses))
        assert torch.equal(flats[0][0], flats[1][0]) and flats[0][1] == flats[1][1]
        assert not torch.equal(flats[0][0], _Head(7, 4).w.detach().reshape(-1).to(dev))


# ------------------------------------------------------------------------------------ tecm_quantile_stats
def _taus(Q):
    return tuple((q + 1) / (Q + 1) for q in range(Q)) if Q != 3 else (0.1, 0.5, 0.9)


def _hard_levels(S, Q, H, I, rng):
    """Scaled levels (unsorted: crossings) and truths with exact ties between levels and with the truth, NaN and both
    infinities in both operands, and values the clip of a scaled run catches (-30 -> below 0 TECU, +40 -> above 200)."""
    lv = (rng.standard_normal((S, Q, H, I)) * 2.5).astype(np.float32)
    if rng.random() < 0.5:
        lv = np.sort(lv, axis=1)                                           # mostly monotone: crossings are the exception
        swap = rng.random((S, H, I)) < 0.2
        if Q > 1:
            a, b = lv[:, 0].copy(), lv[:, Q - 1].copy()
            lv[:, 0], lv[:, Q - 1] = np.where(swap, b, a), np.where(swap, a, b)
    t = (rng.standard_normal((S, H, I)) * 2.5).astype(np.float32)
    if Q > 1:
        tie = rng.random((S, H, I)) < 0.15
        lv[:, 1] = np.where(tie, lv[:, 0], lv[:, 1])                       # two levels equal
    on = rng.random((S, H, I)) < 0.15
    t = np.where(on, lv[:, Q // 2], t).astype(np.float32)                  # the truth exactly on a level
    lv[rng.random(lv.shape) < 0.05] = np.float32(-30.0)
    lv[rng.random(lv.shape) < 0.05] = np.float32(+40.0)
    for a in (lv.reshape(-1), t.reshape(-1)):
        if a.size >= 6:
            w = rng.choice(a.size, size=3, replace=False)
            a[w[0]], a[w[1]], a[w[2]] = np.nan, np.inf, -np.inf
    return lv, t


def _levels_on(lv, layout, dev):
    """(S, Q, H, I) numpy -> a device view of that shape: node-contiguous, or horizon-fastest (the model's (B, N, Q * H))."""
    d = torch.from_numpy(lv).to(dev)
    if layout == "h_fast":
        S, Q, H, I = lv.shape
        d = d.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    return d


def _assert_sums(got, want, mags, what):
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    err = np.abs(got[fin] - want[fin])
    worst = float(np.max(err / np.maximum(mags[fin], 1e-300))) if err.size else 0.0
    print(f"{what}: max |kernel - numpy| / sum|terms| = {worst:.3e}")
    assert np.all(err <= BAR * mags[fin]), (what, worst)


@pytest.mark.parametrize("H", [1, 12, 24])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 135])
def test_quantile_stats_match_the_ordered_float64_restatement(dev, N, H):
    """Every Q bucket and its edges x (three groups with ids out of order, group 1 never visited and pre-filled with a sentinel
    that must survive | one group, one sample) x both level layouts x scaler + clip + adjust on / off; two updates into one
    object against the restatement of both and against one update on the concatenation; the sorted per-sample output."""
    from src.evaluation.metrics import QuantileMetrics
    from tecmollm import check_device_errors
    rng = np.random.default_rng(11 * N + H)
    for Q in (1, 2, 3, 5, 9, 16):
        taus, rows = _taus(Q), 1 + Q + Q // 2
        for variant in range(3):
            # 0: three groups, scaler + clip, nodes contiguous, an adjust per group;  1: three groups, no scaler, horizon-fastest,
            # one adjust for all;  2: one group, one sample, scaler, no adjust
            S, G = (5, 3) if variant < 2 else (1, 1)
            scaler = SCALER if variant != 1 else None
            layout = "nodes" if variant != 1 else "h_fast"
            Ga = (G, 1, None)[variant]
            adj = None if Ga is None else (rng.standard_normal((Ga, H, Q, N)) * 2).astype(np.float32)
            adj_d = None if adj is None else torch.from_numpy(adj).to(dev)
            what = (N, H, Q, variant)
            qm, one = QuantileMetrics(H, N, taus, G, scaler, dev), QuantileMetrics(H, N, taus, G, scaler, dev)
            if G > 1:
                qm.stats[1].copy_(torch.arange(H * rows * N, device=dev, dtype=torch.float64).view(H, rows, N) + 0.5)
                qm.counts[1].fill_(77)
            want, mags, cnt = np.zeros((G, H, rows, N)), np.zeros((G, H, rows, N)), np.zeros((G, H, rows, N), np.int64)
            batches = []
            for update in range(2):
                lv, t = _hard_levels(S, Q, H, N, rng)
                ids = None if G == 1 else np.array([2, 0, 2, 0, 2] if update == 0 else [0, 2, 2, 0, 0], dtype=np.int32)
                ids_d = None if ids is None else torch.from_numpy(ids).to(dev)
                z = qm.update(_levels_on(lv, layout, dev), torch.from_numpy(t).to(dev).unsqueeze(-1), ids_d, adj_d,
                              want_sorted=update == 0)
                zr = QR.accumulate(want, cnt, mags, lv, t, taus, ids, scaler, adj)
                if update == 0:
                    assert np.array_equal(z.cpu().numpy(), zr, equal_nan=True), what
                    if adj is None:
                        assert np.array_equal(zr, np.sort(QR.values(lv, t, scaler)[0], axis=1)), what
                else:
                    assert z is None
                batches.append((lv, t, ids))
            if G > 1:
                assert (qm.stats[1].cpu().numpy().reshape(-1) == np.arange(H * rows * N) + 0.5).all(), "group 1 was touched"
                assert (qm.counts[1] == 77).all()
                qm.stats[1].zero_()
                qm.counts[1].zero_()
            got, got_c = qm.stats.cpu().numpy(), qm.counts.cpu().numpy()
            assert np.array_equal(got_c, cnt), what
            _assert_sums(got, want, mags, repr(what))
            assert got[:, :, 0].sum() == 2 * S * H * N
            if Q > 1 and S * H * N >= 60:
                assert cnt[:, :, 0].sum() > 0                              # the inputs do cross
            # one update on the concatenation: the same counts, the sums at the bar (another grouping of the additions)
            lv2, t2 = np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches])
            ids2 = None if G == 1 else torch.from_numpy(np.concatenate([b[2] for b in batches])).to(dev)
            one.update(_levels_on(lv2, layout, dev), torch.from_numpy(t2).to(dev), ids2, adj_d)
            assert torch.equal(one.counts, qm.counts), what
            _assert_sums(one.stats.cpu().numpy(), want, mags, repr(what) + " concatenated")
    check_device_errors()


def test_quantile_stats_are_reproducible_report_bad_ids_and_serve_the_forecast_path(dev):
    from src.evaluation.metrics import QuantileMetrics
    from tecmollm import TecmError, check_device_errors
    S, Q, H, N, G = 5, 5, 12, 135, 3
    rng = np.random.default_rng(3)
    lv, t = _hard_levels(S, Q, H, N, rng)
    taus = _taus(Q)
    lv_d, t_d = _levels_on(lv, "h_fast", dev), torch.from_numpy(t).to(dev)
    ids = torch.tensor([2, 0, 1, 0, 2], dtype=torch.int32, device=dev)
    runs = []
    for _ in range(3):
        qm = QuantileMetrics(H, N, taus, G, SCALER, dev)
        z = qm.update(lv_d, t_d, ids, want_sorted=True)
        runs.append((qm.stats.clone(), qm.counts.clone(), z))
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r[:2], runs[0][:2])) and torch.equal(r[2], runs[0][2])
    # the forecast path: no truth, nothing accumulated, the same sorted levels
    fc = QuantileMetrics(H, N, taus, G, SCALER, dev)
    zf = fc.update(lv_d, None, ids)
    assert torch.equal(zf, runs[0][2]) and fc.stats.abs().sum() == 0 and fc.counts.abs().sum() == 0
    assert (zf[:, 1:] >= zf[:, :-1]).all() and (zf >= 0).all() and (zf <= 200).all()
    # a bad id: the sample is skipped, the word is set
    bad = QuantileMetrics(H, N, taus, G, SCALER, dev)
    bad.update(lv_d, t_d, torch.tensor([2, 0, 3, 0, -1], dtype=torch.int32, device=dev))
    with pytest.raises(TecmError, match="TECM_BAD_GROUP"):
        check_device_errors()
    check_device_errors()
    want, mags, cnt = (np.zeros((G, H, 1 + Q + Q // 2, N)) for _ in range(3))
    cnt = cnt.astype(np.int64)
    QR.accumulate(want, cnt, mags, lv, t, taus, np.array([2, 0, 3, 0, -1]), SCALER)
    assert np.array_equal(bad.counts.cpu().numpy(), cnt) and bad.stats[:, :, 0].sum().item() == 3 * H * N
    _assert_sums(bad.stats.cpu().numpy(), want, mags, "bad ids")


# ------------------------------------------------------------------------------------ CQR
class _Table(torch.nn.Module):
    """A stand-in forecaster: x holds window indices, the output is that row of a table of (Q * H, N) forecasts, handed out
    as the model's permuted (B, Q * H, N, 1) view."""

    def __init__(self, table):                                             # (S, Q, H, N) on the device
        super().__init__()
        S, Q, H, N = table.shape
        self.storage = table.permute(0, 3, 1, 2).reshape(S, N, Q * H).contiguous()

    def forward(self, x, tf, ei, ew=None):
        return self.storage[x].permute(0, 2, 1).unsqueeze(-1)


class _Windows:
    def __init__(self, y):                                                 # (S, H, N) on the device
        self.y = y

    def __len__(self):
        return self.y.shape[0]

    def batch(self, chunk):
        idx = torch.as_tensor(list(chunk), dtype=torch.int64, device=self.y.device)
        return idx, None, self.y[idx].unsqueeze(-1)


@pytest.mark.parametrize("H", [1, 12])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 135])
def test_quantile_scores_are_the_restatement_exactly(dev, N, H):
    from tecmollm import ops
    S, row0, pad = 5, 2, 3
    rng = np.random.default_rng(5 * N + H)
    for Q, pair in ((1, (0, 0)), (2, (0, 1)), (3, (0, 2)), (5, (1, 3)), (9, (0, 8)), (16, (3, 12))):
        lv, t = _hard_levels(S, Q, H, N, rng)
        for layout, scaler in (("nodes", None), ("h_fast", SCALER)):
            store = torch.full((S + 4, H * N + pad), -777.0, device=dev)
            mean, scale = scaler if scaler else (0.0, 1.0)
            ops.quantile_scores(_levels_on(lv, layout, dev).permute(1, 0, 2, 3), torch.from_numpy(t).to(dev), store, row0,
                                pair[0], pair[1], mean=mean, scale=scale, clip=(0.0, 200.0) if scaler else None)
            want = QR.cqr_scores(lv, t, pair[0], pair[1], scaler).reshape(S, H * N)
            got = store.cpu().numpy()
            assert np.array_equal(got[row0:row0 + S, :H * N], want), (N, H, Q, layout)
            assert (got[:row0] == -777).all() and (got[row0 + S:] == -777).all() and (got[:, H * N:] == -777).all()


def test_calibrate_cqr_selects_the_stated_rank_and_covers_its_calibration_windows(dev):
    """Dyadic levels and truths without a scaler, so E, z_lo - Qhat and z_hi + Qhat are exact and E <= Qhat is exactly
    "covered": per cell at least rank of the n calibration windows of a group are covered.  Group 2 has 3 windows, too few
    for alpha = 0.25 (rank ceil(4 * 0.75) = 3 -- enough) but not group 1 with 2 (rank 3 > 2): infinite."""
    from src.evaluation.metrics import QuantileMetrics
    from tecmollm import QuantileModel, calibrate_cqr, conformal_ranks
    S, H, N, G = 23, 3, 65, 3
    taus, pair = (0.125, 0.5, 0.875), (0.125, 0.875)
    g = torch.Generator().manual_seed(9)
    lv = torch.randint(-20, 21, (S, 3, H, N), generator=g).float() * 0.25  # unsorted: the scores use the sorted levels
    y = torch.randint(-24, 25, (S, H, N), generator=g).float() * 0.25
    ids = np.array([0] * 18 + [1] * 2 + [2] * 3, dtype=np.int32)
    ids = ids[np.random.default_rng(1).permutation(S)]
    qmodel = QuantileModel(_Table(lv.to(dev)), taus, H)
    ds = _Windows(y.to(dev))
    iv = calibrate_cqr(qmodel, ds, None, 5, pair=pair, groups=torch.from_numpy(ids).to(dev), num_groups=G)
    assert iv.alpha == 0.25 and iv.pair == pair and iv.counts.tolist() == [18, 2, 3] and iv.offset.shape == (G, H, N)
    assert not iv.finite and np.isposinf(iv.offset[1]).all() and np.isfinite(iv.offset[[0, 2]]).all() and iv.scaler is None
    E = QR.cqr_scores(lv.numpy(), y.numpy(), 0, 2, None)
    for grp in (0, 2):
        n = int((ids == grp).sum())
        rank = conformal_ranks(n, 0.25, "absolute")[0]
        assert rank == {18: 15, 3: 3}[n]
        assert np.array_equal(iv.offset[grp], np.sort(E[ids == grp], axis=0)[rank - 1]), grp
    qm = QuantileMetrics(H, N, taus, G, None, dev)
    qm.update(qmodel.quantiles(torch.arange(S, device=dev), None, None), y.to(dev), torch.from_numpy(ids).to(dev), iv.on(dev))
    covered = qm.counts[:, :, 1 + 3].cpu().numpy()
    assert (covered[0] >= 15).all() and (covered[2] >= 3).all() and (covered[1] == 2).all()      # +-inf covers everything
    # a single group, one call
    one = calibrate_cqr(qmodel, ds, None, 7, pair=pair)
    assert one.finite and np.array_equal(one.offset[0], np.sort(E, axis=0)[conformal_ranks(S, 0.25, "absolute")[0] - 1])
    with pytest.raises(ValueError, match="pair"):
        calibrate_cqr(qmodel, ds, None, 7, pair=(0.1, 0.9))


def test_cqr_of_equal_levels_degenerates_to_absolute_split_conformal(dev):
    from tecmollm import QuantileModel, calibrate_conformal, calibrate_cqr
    S, H, N = 19, 2, 64
    g = torch.Generator().manual_seed(4)
    point = torch.randn(S, 1, H, N, generator=g)
    y = torch.randn(S, H, N, generator=g).to(dev)
    ids = (torch.arange(S) % 2).to(torch.int32).to(dev)
    qmodel = QuantileModel(_Table(point.expand(S, 3, H, N).contiguous().to(dev)), (0.05, 0.5, 0.95), H)
    ds = _Windows(y)
    for scaler in (None, SCALER):
        iv = calibrate_cqr(qmodel, ds, None, 4, pair=(0.05, 0.95), scaler=scaler, groups=ids, num_groups=2)
        ref = calibrate_conformal(qmodel, ds, None, 4, alpha=0.1, scaler=scaler, groups=ids, num_groups=2, mode="absolute")
        assert abs(iv.alpha - 0.1) < 1e-15 and iv.counts.tolist() == ref.counts.tolist()
        assert np.array_equal(iv.offset, ref.q_hi), scaler


# ------------------------------------------------------------------------------------ end to end
KEYS = ("mae_avg", "rmse_avg", "r2_score_avg", "pearson_r_avg", "mae_by_horizon", "rmse_by_horizon", "r2_by_horizon",
        "pearson_by_horizon")
TAUS = (0.1, 0.5, 0.9)


@pytest.fixture(scope="module")
def split(dev, golden_dir):
    from oracle import ref_cpu as R
    from src.data.dataset import SlidingWindowSamplerDataset
    from tecmollm import QuantileModel, quantile_config
    from tests.parity import build_model
    cfg = quantile_config(R.default_config(L_in=16, L_out=12, num_nodes=12), TAUS)
    assert cfg["prediction_horizon"] == 36
    model = build_model(cfg, R.init_params(cfg, seed=3), dev, "per_timestep")
    g = np.load(os.path.join(golden_dir, "evaluate_split.npz"))
    ds = SlidingWindowSamplerDataset.from_tensors(torch.as_tensor(g["X"]), torch.as_tensor(g["Y"]), torch.as_tensor(g["TF"]),
                                                  int(g["L_in"]), int(g["L_out"]), stride=1, device=dev, mode="test")
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev)
    return QuantileModel(model, TAUS, 12).eval(), ds, ei, (float(g["mean"]), float(g["scale"]))


def test_quantiles_end_to_end_on_a_tiny_model(dev, split, tmp_path):
    """12 nodes, 24 windows, batch size 5 (a ragged last batch), an untrained three-level model."""
    from src.evaluation.metrics import MAP_KEYS, QUANTILE_KEYS
    from tecmollm import calibrate_cqr, evaluate_quantiles, quantile_forecast, write_quantiles
    from tecmollm import evaluate as E
    qmodel, ds, ei, scaler = split
    S, N, H = len(ds), 12, 12
    slots = (torch.arange(S, device=dev) % 3).to(torch.int32)
    kw = dict(scaler=scaler, baselines=("mean", "last"), groups=slots, num_groups=3)
    want_res, want_maps = E.evaluate_maps(qmodel, ds, ei, 5, **kw)
    res, maps, quant = evaluate_quantiles(qmodel, ds, ei, 5, **kw)
    assert list(res) == list(want_res) and list(maps) == list(want_maps)
    for name in want_res:
        for k in KEYS:
            assert res[name][k] == want_res[name][k], (name, k)
        for k in MAP_KEYS:
            assert np.array_equal(maps[name][k], want_maps[name][k], equal_nan=True), (name, k)
    plain = E.evaluate_split(qmodel, ds, ei, 5, scaler=scaler, baselines=("mean", "last"))
    assert all(plain[name][k] == want_res[name][k] for name in want_res for k in KEYS)
    assert set(quant) == set(QUANTILE_KEYS) | {"taus", "pairs", "by_group"}
    assert quant["count"].shape == (3, H, N) and quant["count"].sum() == S * H * N and (quant["count"][0] == 8).all()
    assert quant["pinball"].shape == (3, H, N, 3) and quant["coverage"].shape == (3, H, N, 1)
    assert ((quant["reliability"][..., 1:] >= quant["reliability"][..., :-1]).all())               # sorted levels
    assert np.isfinite(quant["quantile_crps"]).all() and (quant["crossing_rate"] >= 0).all()
    # the two halves of the split, added by hand
    a = evaluate_quantiles(qmodel, ds, ei, 5, order=list(range(0, 11)), **kw)[2]
    b = evaluate_quantiles(qmodel, ds, ei, 5, order=list(range(11, S)), **kw)[2]
    na, nb = np.nan_to_num(a["count"]), np.nan_to_num(b["count"])
    assert np.array_equal(na + nb, quant["count"])
    for k in QUANTILE_KEYS[1:]:
        wa, wb = (na, nb) if quant[k].ndim == 3 else (na[..., None], nb[..., None])
        both = (np.nan_to_num(a[k]) * wa + np.nan_to_num(b[k]) * wb) / (wa + wb)
        np.testing.assert_allclose(both, quant[k], rtol=1e-12, atol=1e-12, err_msg=k)
    # the files
    paths = write_quantiles(quant, str(tmp_path / "out"), grid=(3, 4))
    z = np.load(paths["npz"])
    assert z["pinball"].shape == (3, H, 3, 4, 3) and np.array_equal(z["coverage"].reshape(3, H, N, 1), quant["coverage"])
    with open(paths["csv"], encoding="utf-8") as f:
        assert len(f.read().splitlines()) == 1 + 3 * H
    # CQR on the first 14 windows: scoring them with the offsets covers at least rank 12 of 14 in every cell
    cal = list(range(14))
    iv = calibrate_cqr(qmodel, ds, ei, 5, pair=(0.1, 0.9), scaler=scaler, order=cal)
    assert qmodel.training is False and iv.finite and iv.counts.tolist() == [14] and iv.offset.shape == (1, H, N)
    own = evaluate_quantiles(qmodel, ds, ei, 5, scaler=scaler, intervals=iv, order=cal)[2]
    # rank ceil(15 * 0.8) = 12 of the 14 scores are <= the offset; with non-dyadic values fl(z_lo - offset) <= y may fail where
    # E == offset to the last bit, i.e. for the window(s) of that rank alone: at least 11 of 14 (the exact inequality is
    # asserted on dyadic inputs in test_calibrate_cqr_selects_the_stated_rank_and_covers_its_calibration_windows)
    assert own["count"].sum() == 14 * H * N and (own["coverage"][..., 0] * 14 >= 11 - 1e-9).all()
    x, tf, y = ds.batch([20, 21])
    fc = quantile_forecast(qmodel, x, tf, ei, scaler)
    assert set(fc) == {"quantiles", "median"} and fc["quantiles"].shape == (2, 3, H, N) and fc["median"].shape == (2, H, N)
    assert (fc["quantiles"][:, 1:] >= fc["quantiles"][:, :-1]).all() and (fc["quantiles"] >= 0).all()
    fi = quantile_forecast(qmodel, x, tf, ei, intervals=iv)
    assert set(fi) == {"quantiles", "median", "lo", "hi"} and torch.equal(fi["median"], fc["median"])
    off = torch.from_numpy(iv.offset[0]).to(dev)
    assert torch.equal(fi["lo"], fc["quantiles"][:, 0] - off) and torch.equal(fi["hi"], fc["quantiles"][:, 2] + off)


# ------------------------------------------------------------------------------------ rank merge
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_sums(rank):
    g = torch.Generator().manual_seed(60 + rank)
    return (torch.rand((2, 3, 5, 6), generator=g, dtype=torch.float64) * 100,
            torch.randint(0, 1 << 20, (2, 3, 5, 6), generator=g, dtype=torch.int32))


def _merge_worker(rank, port, out_dir):
    import sys
    import torch.distributed as dist
    for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from src.evaluation.metrics import QuantileMetrics
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    try:
        qm = QuantileMetrics(3, 6, (0.1, 0.5, 0.9), 2, None, device="cpu")
        st, ct = _rank_sums(rank)
        qm.stats.copy_(st)
        qm.counts.copy_(ct)
        assert qm.merge_() is qm
        torch.save({"stats": qm.stats, "counts": qm.counts}, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_merge_on_two_gloo_ranks_is_the_plain_sum(tmp_path):
    """The statistics of two ranks (host tensors: the ranks open no GPU) after `merge_`: the plain sum, on both ranks."""
    import torch.multiprocessing as mp
    mp.spawn(_merge_worker, args=(_free_port(), str(tmp_path)), nprocs=2, join=True)
    (s0, c0), (s1, c1) = _rank_sums(0), _rank_sums(1)
    for rank in (0, 1):
        got = torch.load(os.path.join(tmp_path, f"rank{rank}.pt"))
        assert torch.equal(got["stats"], s0 + s1) and torch.equal(got["counts"], c0 + c1) and got["counts"].dtype == torch.int32
