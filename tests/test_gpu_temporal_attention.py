"""GPU tests of the temporal attention maps (csrc/attention_probs.hip through tecmollm/temporal_attention.py): the exported
probabilities against the float64 causal softmax (tests/temporal_attention_ref.py, tied to the frozen oracle by
tests/test_host_temporal_attention.py) at every T either side of the kernels' edges, with NaN in the unread q_0, on hard rows,
against the production forward's context, for node lists, the fp64 accumulator and its groups, across workspace chunks, through
the model (fp32 and bf16), `LLMBackbone.forward(output_attentions=True)`, `evaluate_temporal_attention` and the full grid.

Bars.  p: |kernel - float64| <= parity.RTOL * |float64| + 1e-12, the project's bar for exported coefficients (an fp32
restatement on the CPU sits at 1.1e-3 of it at N(0, 1) inputs, 1.6e-2 on the hard rows: the printed worst ratio should be far
below 1).  A row sums to 1 within (i + 2) * 2^-24, summed in float64: the denominator is the fp32 sum of exactly the i + 1
numerators that are divided.  The statistics are a pure function of the export: against ordered float64 loops over the exported
fp32 p every cell is within n * 2^-52 relative, n = the number of probabilities added into it (all terms are non-negative, so
this bounds any summation order: each side is off by at most (n - 1) 2^-53, the division by T adds 2^-53 per side and window),
plus 1e-12 for the entropy cells' float64 logarithm."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import parity
from tests import spatial_attention_ref as A
from tests import temporal_attention_ref as TA

pytestmark = pytest.mark.gpu

H, D = 12, 768
U24, U52 = 2.0 ** -24, 2.0 ** -52
_models = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _qkv(B, T, N, seed=0, scale=1.0):
    qkv = torch.randn(B * T * N, 3 * D, generator=torch.Generator().manual_seed(1000 + seed))
    qkv[:, :2 * D] *= scale
    return qkv


def _export(qkv_dev, B, T, N, nodes=None, fill=None):
    from tecmollm import ops
    Ns = N if nodes is None else len(nodes)
    probs = torch.empty(B, Ns, H, T, T, device=qkv_dev.device, dtype=torch.float32)
    if fill is not None:
        probs.fill_(fill)
    nd = None if nodes is None else torch.tensor(nodes, dtype=torch.int32, device=qkv_dev.device)
    ops.temporal_attention(qkv_dev, B, T, N, H, D, probs=probs, nodes=nd)
    return probs


def _assert_probs(got, want, what, floor=None):
    """The bar on every entry (or, with `floor`, on the entries whose reference is >= floor); prints the worst ratio."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ratio = np.abs(got - want) / (parity.RTOL * np.abs(want) + 1e-12)
    if floor is not None:
        ratio = np.where(want >= floor, ratio, 0.0)
    worst = float(ratio.max())
    print(f"{what}: max |kernel - float64| / (RTOL |float64| + 1e-12) = {worst:.3e}")
    assert worst <= 1.0, (what, worst)


def _assert_distributions(got, what):
    """Exact zeros beyond the diagonal, row 0 exactly [1, 0, ...], every row sums to 1 within (i + 2) 2^-24 in float64."""
    got = np.asarray(got)
    T = got.shape[-1]
    assert got.dtype == np.float32 and np.isfinite(got).all(), what
    upper = np.triu(np.ones((T, T), bool), 1)
    assert (got[..., upper] == 0).all() and not np.signbit(got[..., upper]).any(), what
    assert (got[..., 0, 0] == 1).all() and (got[..., 0, 1:] == 0).all(), what
    dev_ = np.abs(got.astype(np.float64).sum(-1) - 1.0) / ((np.arange(T) + 2) * U24)
    print(f"{what}: max |row sum - 1| / ((i + 2) 2^-24) = {float(dev_.max()):.3f}")
    assert dev_.max() <= 1.0, (what, float(dev_.max()))


# ------------------------------------------------------------------------------------ 1. the kernel against float64
@pytest.mark.parametrize("T", [1, 2, 3, 4, 6, 12, 13, 21, 24, 25, 32, 33, 64, 65, 90, 1024])
def test_probs_match_float64(dev, T):
    B, N = (1, 2) if T == 1024 else (2, 5)          # 120 (sequence, head) items: the last block of either kernel is not full
    qkv = _qkv(B, T, N, seed=T)
    got = _export(qkv.to(dev), B, T, N).cpu().numpy()
    assert got.shape == (B, N, H, T, T)
    _assert_probs(got, TA.causal_probs(qkv.numpy(), B, T, N), f"fp32 qkv T={T}")
    _assert_distributions(got, f"fp32 qkv T={T}")


@pytest.mark.parametrize("T", [3, 21, 36])
def test_probs_match_float64_bf16_qkv(dev, T):
    B, N = 2, 5
    q16 = _qkv(B, T, N, seed=50 + T).to(torch.bfloat16)
    got = _export(q16.to(dev), B, T, N).cpu().numpy()
    _assert_probs(got, TA.causal_probs(q16.double().numpy(), B, T, N), f"bf16 qkv T={T}")
    _assert_distributions(got, f"bf16 qkv T={T}")


# ------------------------------------------------------------------------------------ 2. q_0 is not read
@pytest.mark.parametrize("T", [3, 21, 36])
def test_q0_is_never_read(dev, T):
    B, N = 2, 5
    qkv = _qkv(B, T, N, seed=70 + T)
    want = _export(qkv.to(dev), B, T, N)
    poisoned = qkv.view(B, T, N, 3 * D).clone()
    poisoned[:, 0, :, :D] = float("nan")
    got = _export(poisoned.view(B * T * N, 3 * D).to(dev), B, T, N)
    assert torch.equal(got, want)
    assert torch.equal(_export(poisoned.view(B * T * N, 3 * D).to(torch.bfloat16).to(dev), B, T, N),
                       _export(qkv.to(torch.bfloat16).to(dev), B, T, N))


# ------------------------------------------------------------------------------------ 3. hard rows
@pytest.mark.parametrize("T", [6, 21, 36, 90])
def test_hard_rows(dev, T):
    """q and k x 4: logits spread over hundreds inside a row, fp32 underflows to exact zeros.  Everything finite, entries with
    reference >= 1e-6 inside the bar, smaller ones < 2e-6, the argmax of every row the reference's."""
    B, N = 2, 5
    qkv = _qkv(B, T, N, seed=90 + T, scale=4.0)
    got = _export(qkv.to(dev), B, T, N).cpu().numpy()
    want = TA.causal_probs(qkv.numpy(), B, T, N)
    _assert_distributions(got, f"hard T={T}")
    _assert_probs(got, want, f"hard T={T}, reference >= 1e-6", floor=1e-6)
    assert (got[want < 1e-6] < 2e-6).all()
    assert np.array_equal(got.argmax(-1), want.argmax(-1))


# ------------------------------------------------------------------------------------ 4. tie to the production forward
@pytest.mark.parametrize("T", [3, 21, 36])
def test_export_reproduces_the_production_context(dev, T):
    from tecmollm import ops
    B, N = 2, 5
    qkv = _qkv(B, T, N, seed=110 + T)
    qd = qkv.to(dev)
    ctx = torch.empty(B * T * N, D, device=dev)
    ops.attention_fwd(qd, ctx, B, T, N, H, D)
    p = _export(qd, B, T, N).cpu().double().numpy()
    want = p @ TA.values_of(qkv.numpy(), B, T, N)                                # (B, N, H, T, hd)
    want = torch.from_numpy(want.transpose(0, 3, 1, 2, 4).reshape(B * T * N, D))
    parity.assert_close(ctx.cpu(), want, f"ctx from the exported p, T={T}")


# ------------------------------------------------------------------------------------ 5. node lists
@pytest.mark.parametrize("T", [6, 36])
def test_node_list_is_a_slice_of_the_full_export(dev, T):
    B, N = 2, 5
    qd = _qkv(B, T, N, seed=130 + T).to(dev)
    full = _export(qd, B, T, N)
    assert torch.equal(_export(qd, B, T, N, nodes=[4, 0, 2]), full[:, [4, 0, 2]])
    got = _export(qd, B, T, N, nodes=[1, N, 3, -1], fill=7.0)                   # ids outside [0, N): the slot stays zero
    assert torch.equal(got[:, [0, 2]], full[:, [1, 3]]) and (got[:, [1, 3]] == 0).all()


# ------------------------------------------------------------------------------------ 6. the statistics
def _buffers(dev, G, Ly, N, T, matrix=True):
    return dict(node_stats=torch.zeros(G, Ly, 4, N, H, device=dev, dtype=torch.float64),
                lag_stats=torch.zeros(G, Ly, H, T, device=dev, dtype=torch.float64),
                matrix_stats=torch.zeros(G, Ly, H, T, T, device=dev, dtype=torch.float64) if matrix else None,
                counts=torch.zeros(G, device=dev, dtype=torch.int64))


def _assert_stats(node, lag, mat, counts, probs, groups, G, what, fast=False):
    """node (G, 4, N, H), lag (G, H, T), mat (G, H, T, T) or None, counts (G) of the device against the float64 loops over the
    exported fp32 `probs` (B, N, H, T, T)."""
    probs = np.asarray(probs)
    _, N, _, T, _ = probs.shape
    wn, wl, wm, wc = (TA.accumulate_fast if fast else TA.accumulate_ref)(probs, groups, G)
    assert np.asarray(counts).tolist() == wc.tolist(), what
    worst = 0.0
    for g in range(G):
        W = int(wc[g])
        if W == 0:
            assert (np.asarray(node)[g] == 0).all() and (np.asarray(lag)[g] == 0).all(), what
            assert mat is None or (np.asarray(mat)[g] == 0).all(), what
            continue
        tri = T * (T + 1) // 2
        for k, (terms, extra) in enumerate(((tri, 1e-12), (tri, 0.0), (T, 0.0), (T, 0.0))):
            bar = (W * terms * U52 + extra) * np.abs(wn[g, k])
            err = np.abs(np.asarray(node)[g, k] - wn[g, k])
            assert (err <= bar).all(), (what, "node", g, k, float((err / np.maximum(bar, 1e-300)).max()))
            worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
        bar = W * N * (T - np.arange(T)) * U52 * np.abs(wl[g])
        err = np.abs(np.asarray(lag)[g] - wl[g])
        assert (err <= bar).all(), (what, "lag", g)
        worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
        if mat is not None:
            err = np.abs(np.asarray(mat)[g] - wm[g])
            assert (err <= W * N * U52 * np.abs(wm[g])).all(), (what, "matrix", g)
    print(f"{what}: worst |device - loops| / bar = {worst:.3f}")


@pytest.mark.parametrize("T", [3, 6, 21, 32, 36, 65])
def test_statistics_are_a_function_of_the_export(dev, T):
    """Three groups, one of them empty; export and statistics from one call."""
    from tecmollm import ops
    B, N, G = 2, 5, 3
    qd = _qkv(B, T, N, seed=150 + T).to(dev)
    groups = [2, 0]
    buf = _buffers(dev, G, 2, N, T, matrix=T <= 32)
    probs = torch.empty(B, N, H, T, T, device=dev)
    ops.temporal_attention(qd, B, T, N, H, D, probs=probs, groups=torch.tensor(groups, dtype=torch.int32, device=dev), layer=1,
                           count=True, **buf)
    assert torch.equal(probs, _export(qd, B, T, N))
    for k in ("node_stats", "lag_stats", "matrix_stats"):
        assert buf[k] is None or (buf[k][:, 0] == 0).all()                       # layer slot 0 untouched
    mat = buf["matrix_stats"][:, 1].cpu().numpy() if T <= 32 else None
    _assert_stats(buf["node_stats"][:, 1].cpu().numpy(), buf["lag_stats"][:, 1].cpu().numpy(), mat,
                  buf["counts"].cpu().numpy(), probs.cpu().numpy(), groups, G, f"statistics T={T}")
    # a second call adds on top; without `count` the counts stay
    ops.temporal_attention(qd, B, T, N, H, D, groups=torch.tensor(groups, dtype=torch.int32, device=dev), layer=1, **buf)
    assert buf["counts"].tolist() == [1, 0, 1]
    twice = np.concatenate([probs.cpu().numpy()] * 2)
    wn = TA.accumulate_fast(twice, groups * 2, G)[0]
    np.testing.assert_allclose(buf["node_stats"][:, 1].cpu().numpy(), wn, rtol=1e-11, atol=0)
    # with a node list next to the statistics the export is that list, the statistics those of all nodes
    buf2 = _buffers(dev, G, 2, N, T, matrix=T <= 32)
    sub = torch.empty(B, 2, H, T, T, device=dev)
    ops.temporal_attention(qd, B, T, N, H, D, probs=sub, nodes=torch.tensor([3, 1], dtype=torch.int32, device=dev),
                           groups=torch.tensor(groups, dtype=torch.int32, device=dev), layer=1, count=True, **buf2)
    assert torch.equal(sub, probs[:, [3, 1]])
    buf3 = _buffers(dev, G, 2, N, T, matrix=T <= 32)
    ops.temporal_attention(qd, B, T, N, H, D, groups=torch.tensor(groups, dtype=torch.int32, device=dev), layer=1, count=True,
                           **buf3)
    for k in ("node_stats", "lag_stats", "matrix_stats", "counts"):
        assert buf2[k] is None or torch.equal(buf2[k], buf3[k]), k


@pytest.mark.parametrize("T", [6, 36])
def test_a_bad_group_id_skips_the_window_and_raises(dev, T):
    from tecmollm import TecmError, check_device_errors, devcheck, ops
    B, N, G = 2, 5, 2
    qd = _qkv(B, T, N, seed=170 + T).to(dev)
    check_device_errors(dev)
    errs = devcheck.error_word(dev)
    buf = _buffers(dev, G, 1, N, T, matrix=T <= 32)
    probs = torch.empty(B, N, H, T, T, device=dev)
    for groups in ([1, 5], [1, -1]):
        ops.temporal_attention(qd, B, T, N, H, D, probs=probs, groups=torch.tensor(groups, dtype=torch.int32, device=dev),
                               count=True, err_flag=errs.ptr(), **buf)
        errs.post()
        with pytest.raises(TecmError, match="TECM_BAD_GROUP"):
            check_device_errors(dev)
    mat = buf["matrix_stats"][:, 0].cpu().numpy() if T <= 32 else None
    twice = np.concatenate([probs.cpu().numpy()] * 2)
    _assert_stats(buf["node_stats"][:, 0].cpu().numpy(), buf["lag_stats"][:, 0].cpu().numpy(), mat, buf["counts"].cpu().numpy(),
                  twice, [1, 5, 1, -1], G, f"bad group T={T}")
    assert buf["counts"].tolist() == [0, 2]


# ------------------------------------------------------------------------------------ 7. chunking and determinism
@pytest.mark.parametrize("T", [6, 36])
def test_chunks_and_repeats_give_the_same_bits(dev, T):
    """Four windows through a workspace that holds one: four chunks, the bits of the default workspace."""
    from tecmollm import ops
    B, N, G = 4, 5, 2
    qd = _qkv(B, T, N, seed=190 + T).to(dev)
    groups = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device=dev)
    one_window = ops.temporal_attention_ws_floats(1, T, N, H, D, True, T <= 32) * 4
    assert ops.temporal_attention_ws_floats(B, T, N, H, D, True, T <= 32) * 4 == B * one_window

    def run(cap):
        buf = _buffers(dev, G, 1, N, T, matrix=T <= 32)
        probs = torch.empty(B, N, H, T, T, device=dev)
        ops.temporal_attention(qd, B, T, N, H, D, probs=probs, groups=groups, count=True, max_ws_bytes=cap, **buf)
        return [probs] + [buf[k] for k in ("node_stats", "lag_stats", "matrix_stats", "counts") if buf[k] is not None]

    want = run(None)
    for cap in (None, one_window, one_window + 8):
        for a, b in zip(run(cap), want):
            assert torch.equal(a, b), cap
    assert want[-1].tolist() == [2, 2]
    from tecmollm import TecmError
    with pytest.raises(TecmError, match="one window needs"):
        run(one_window - 8)


# ------------------------------------------------------------------------------------ 8. through the model
N_MODEL, B_MODEL = 20, 2
EI = A.irregular_graph(N_MODEL)


def _config(which, num_nodes=N_MODEL, llm_layers=2):
    cfg = R.default_config(L_in={"T3": 48, "T6": 96, "T36": 144}[which], L_out=12, num_nodes=num_nodes, llm_layers=llm_layers)
    if which == "T36":
        cfg["patch_len"] = 1
    return cfg


def _model(dev, which, num_nodes=N_MODEL, llm_layers=2, precision=None):
    """(model in eval mode, config, oracle parameters), built once per configuration."""
    key = (which, num_nodes, llm_layers, precision)
    if key not in _models:
        cfg = _config(which, num_nodes, llm_layers)
        params = R.init_params(cfg, seed=31)
        _models[key] = (parity.build_model(cfg, params, dev, precision=precision).eval(), cfg, params)
    return _models[key]


def _inputs(cfg, b=B_MODEL, seed=0):
    g = torch.Generator().manual_seed(300 + seed)
    L, n = cfg["temporal_seq_len"], cfg["num_nodes"]
    x = torch.randn(b, L, n, 6, generator=g)
    tf = torch.stack([torch.randint(0, hi, (b, L, 1), generator=g) for hi in (12, 366, 13, 4)], -1).float()
    return x, tf.expand(b, L, n, 4).contiguous()


@pytest.mark.parametrize("which", ["T3", "T6", "T36"])
def test_through_the_model(dev, which):
    from tecmollm import TemporalAttentionStats, check_device_errors, temporal_attention
    model, cfg, params = _model(dev, which)
    T = model.num_patches
    assert T == int(which[1:])
    x, tf = _inputs(cfg, seed=T)
    xd, tfd, eid = x.to(dev), tf.to(dev), EI.to(dev)
    with torch.no_grad():
        before = model(xd, tfd, eid).clone()
    attn = temporal_attention(model, xd, tfd, eid)
    assert attn.is_cuda and attn.dtype == torch.float32 and attn.shape == (2, B_MODEL, N_MODEL, H, T, T)
    p64 = {k: v.double() for k, v in params.items() if not k.startswith(R.P_HEAD)}
    want = TA.model_attentions(x.double(), tf.double(), EI, p64, cfg)
    for l in range(2):
        _assert_probs(attn[l].cpu().numpy(), want[l].numpy(), f"model {which} block {l}")
        _assert_distributions(attn[l].cpu().numpy(), f"model {which} block {l}")
    assert torch.equal(temporal_attention(model, xd, tfd, eid, layers=[1])[0], attn[1])
    assert torch.equal(temporal_attention(model, xd, tfd, eid, layers=[1, 0], nodes=[7, 19])[1], attn[0][:, [7, 19]])
    model.train()                                    # the pre-dropout probabilities under any training flag, flag left alone
    try:
        assert torch.equal(temporal_attention(model, xd, tfd, eid), attn)
        assert model.training and model.llm_backbone.training
    finally:
        model.eval()
    st = TemporalAttentionStats(N_MODEL, 2, T, device=dev)
    assert st.matrix == (T <= 32)
    pred = st.update(model, xd, tfd, eid)
    with torch.no_grad():
        after = model(xd, tfd, eid)
    assert torch.equal(pred, before) and torch.equal(after, before)
    assert st.counts.tolist() == [B_MODEL]
    for l in range(2):
        mat = st.matrix_stats[:, l].cpu().numpy() if st.matrix else None
        _assert_stats(st.node_stats[:, l].cpu().numpy(), st.lag_stats[:, l].cpu().numpy(), mat, st.counts.cpu().numpy(),
                      attn[l].cpu().numpy(), None, 1, f"model {which} block {l} statistics")
    out = st.compute()
    assert out["entropy"].shape == (1, 2, N_MODEL, H) and out["lag_profile"].shape == (1, 2, H, T)
    assert ("mean" in out) == (T <= 32)
    np.testing.assert_allclose(out["lag_profile"][0, :, :, 0] * T +
                               (out["lag_profile"][0, :, :, 1:] * (T - np.arange(1, T))).sum(-1), T, rtol=1e-6)
    check_device_errors(dev)


def test_counts_advance_once_per_update_with_three_layers_tapped(dev):
    from tecmollm import TemporalAttentionStats
    model, cfg, _ = _model(dev, "T3", llm_layers=3)
    x, tf = _inputs(cfg, seed=5)
    st = TemporalAttentionStats(N_MODEL, 3, 3, num_groups=2, device=dev)
    groups = torch.tensor([1, 1], dtype=torch.int32, device=dev)
    for n in (1, 2):
        st.update(model, x.to(dev), tf.to(dev), EI.to(dev), groups)
        assert st.counts.tolist() == [0, 2 * n]
    assert (st.node_stats[1].abs().sum((1, 2, 3)) > 0).all() and (st.node_stats[0] == 0).all()     # all three layer slots filled
    st.reset()
    assert st.counts.tolist() == [0, 0] and (st.stats == 0).all()


@pytest.mark.parametrize("which", ["T3", "T36"])
def test_backbone_output_attentions(dev, which):
    """`LLMBackbone.forward(h, output_attentions=True)`: the same last_hidden_state bits, Hugging Face's layout, the kernel's
    export of the same qkv, the float64 restatement's probabilities."""
    from tecmollm import functions as F_
    from tecmollm import ops
    model, cfg, params = _model(dev, which)
    bb = model.llm_backbone
    T, S = model.num_patches, 10
    h = torch.randn(S, T, D, generator=torch.Generator().manual_seed(7))
    hd = h.to(dev)
    with torch.no_grad():
        plain = bb(hd)
        out, atts = bb(hd, output_attentions=True)
        taken = {}
        with F_.attention_tap(lambda layer, qkv, B_, T_, N_: taken.__setitem__(layer, (qkv.clone(), B_, T_, N_))):
            assert torch.equal(bb(hd), plain)
    assert isinstance(plain, torch.Tensor) and torch.equal(out, plain)
    assert isinstance(atts, tuple) and len(atts) == 2
    p64 = {k: v.double() for k, v in params.items() if k.startswith(R.P_GPT)}
    want_h, want = TA.gpt2_lora_attentions(h.double(), p64, 2)
    parity.assert_close(out.cpu(), want_h, "last_hidden_state")
    for l in range(2):
        qkv, B_, T_, N_ = taken[l]
        assert (B_, T_, N_) == (S, T, 1) and atts[l].shape == (S, H, T, T) and not atts[l].requires_grad
        assert torch.equal(atts[l], _export(qkv, S, T, 1).view(S, H, T, T))
        _assert_probs(atts[l].cpu().numpy(), want[l].numpy(), f"backbone {which} block {l}")
    # with gradients on and in training mode the hidden state is still the plain forward's (same dropout seed)
    bb.train()
    try:
        with F_.dropout_seed(11):
            torch.manual_seed(3)                                 # the stand-alone front end's embd dropout is torch's
            a = bb(hd)
        with F_.dropout_seed(11):
            torch.manual_seed(3)
            b, atts_t = bb(hd, output_attentions=True)
        assert torch.equal(a, b) and b.requires_grad
        _assert_distributions(atts_t[1].cpu().numpy(), "training-mode attentions are the pre-dropout ones")
    finally:
        bb.eval()


# ------------------------------------------------------------------------------------ 9. the bf16 model
def test_bf16_model(dev):
    from tecmollm import TemporalAttentionStats, temporal_attention
    from tecmollm import functions as F_
    model, cfg, _ = _model(dev, "T6", precision="bf16")
    x, tf = _inputs(cfg, seed=9)
    xd, tfd, eid = x.to(dev), tf.to(dev), EI.to(dev)
    seen = []
    with torch.no_grad(), F_.attention_tap(lambda layer, qkv, *a: seen.append(qkv.dtype)):
        model(xd, tfd, eid)
    assert seen == [torch.bfloat16] * 2                          # the export runs from the bf16 qkv the forward read
    attn = temporal_attention(model, xd, tfd, eid)
    st = TemporalAttentionStats(N_MODEL, 2, 6, device=dev)
    st.update(model, xd, tfd, eid)
    for l in range(2):
        _assert_distributions(attn[l].cpu().numpy(), f"bf16 model block {l}")
        _assert_stats(st.node_stats[:, l].cpu().numpy(), st.lag_stats[:, l].cpu().numpy(), st.matrix_stats[:, l].cpu().numpy(),
                      st.counts.cpu().numpy(), attn[l].cpu().numpy(), None, 1, f"bf16 model block {l} statistics")


# ------------------------------------------------------------------------------------ 10. evaluate_temporal_attention
class _Windows:
    """A device-resident data set of synthetic windows with the `batch` interface the evaluation loops read."""

    def __init__(self, S, l, n, dev):
        from tecmollm.synthetic import synthetic_batch
        x, tf, y = synthetic_batch(S, l, n, 6, 12, seed=21)
        self.x, self.tf, self.y = x.to(dev), tf.contiguous().to(dev), y.to(dev)

    def __len__(self):
        return self.x.shape[0]

    def batch(self, chunk):
        idx = torch.as_tensor(chunk, dtype=torch.int64, device=self.x.device)
        return self.x[idx], self.tf[idx], self.y[idx]


def test_evaluate_temporal_attention_is_the_sum_of_the_exports(dev, tmp_path):
    """Every timestep a graph, so that a window's forward does not depend on which window leads its batch (with
    gat_graphs = "reference" only graph (t = 0, b = 0) of a call aggregates neighbours)."""
    model = _model(dev, "T3")[0]
    model.gat_graphs = model.spatial_encoder.gat_graphs = "per_timestep"
    try:
        _evaluate_case(dev, tmp_path, model)
    finally:
        model.gat_graphs = model.spatial_encoder.gat_graphs = "reference"


def _evaluate_case(dev, tmp_path, model):
    from tecmollm import TecmError, evaluate_temporal_attention, temporal_attention, write_temporal_attention
    from tecmollm.temporal_attention import derive
    S, G, T = 6, 3, 3
    ds = _Windows(S, 48, N_MODEL, dev)
    eid = EI.to(dev)
    ids = [0, 2, 2, 0, 2, 2]                                     # group 1 stays empty
    groups = torch.tensor(ids, dtype=torch.int32, device=dev)
    got = evaluate_temporal_attention(model, ds, eid, 4, groups=groups, num_groups=G)        # batches of 4 and 2
    exports = []
    for a in range(0, S, 4):
        x, tf, _ = ds.batch(list(range(a, min(S, a + 4))))
        exports.append(temporal_attention(model, x, tf, eid).cpu().numpy())
    attn = np.concatenate(exports, 1)                            # (Ly, S, N, H, T, T)
    parts = [TA.accumulate_ref(attn[l], ids, G) for l in range(2)]
    want = derive(np.stack([q[0] for q in parts], 1), np.stack([q[1] for q in parts], 1), parts[0][3],
                  np.stack([q[2] for q in parts], 1))
    assert got["count"].tolist() == [2.0, 0.0, 4.0]
    # another order of the same batches: the windows of each reversed, the ragged batch still last
    rev = evaluate_temporal_attention(model, ds, eid, 4, groups=groups, num_groups=G, order=[3, 2, 1, 0, 5, 4])
    tri = T * (T + 1) // 2
    # terms added into one cell per window: the bar of the sums, which the division by the count leaves as it is; + 1e-12
    # where a logarithm enters; effective_tokens and lookback_gap are functions of two such means
    terms = {"entropy": tri, "lookback": tri, "sink_weight": T, "self_weight": T, "mean": N_MODEL,
             "lag_profile": N_MODEL * (T - np.arange(T))}
    for res in (got, rev):
        assert set(res) == set(want)
        for k in ("entropy", "lookback", "sink_weight", "self_weight", "lookback_gap", "lag_profile", "mean", "effective_tokens"):
            assert np.isnan(res[k][1]).all(), k
            for g, W in ((0, 2), (2, 4)):
                if k in terms:
                    bar = (W * terms[k] * U52 + (1e-12 if k == "entropy" else 0.0)) * np.abs(want[k][g])
                else:
                    bar = 1e-11 * np.abs(want[k][g]) + 1e-13
                assert (np.abs(res[k][g] - want[k][g]) <= bar).all(), (k, g)
    paths = write_temporal_attention(got, str(tmp_path), grid=(4, 5))
    assert sorted(os.path.basename(q) for q in paths.values()) == ["temporal_attention_by_layer.csv",
                                                                   "temporal_attention_maps.npz"]
    z = np.load(paths["npz"])
    assert z["entropy"].shape == (G, 2, H, 4, 5) and z["mean"].shape == (G, 2, H, T, T)
    with pytest.raises(TecmError, match="TECM_BAD_GROUP"):
        evaluate_temporal_attention(model, ds, eid, 4, groups=groups, num_groups=2)
    with pytest.raises(ValueError):
        evaluate_temporal_attention(model, ds, eid, 4, groups=groups[:3], num_groups=G)


# ------------------------------------------------------------------------------------ 11. the full grid, once
def test_full_grid(dev):
    """N = 2911 on the 41 x 71 grid, B = 2, L_in = 48: rows are distributions and the statistics equal the float64 sums over the
    export (vectorised: the same sums in another order, inside the same bar)."""
    from tecmollm import TemporalAttentionStats, temporal_attention
    from tecmollm.synthetic import grid_graph
    n = 2911
    model, cfg, _ = _model(dev, "T3", num_nodes=n)
    x, tf = _inputs(cfg, seed=13)
    xd, tfd, eid = x.to(dev), tf.to(dev), grid_graph()[0].to(dev)
    attn = temporal_attention(model, xd, tfd, eid)
    assert attn.shape == (2, 2, n, H, 3, 3)
    st = TemporalAttentionStats(n, 2, 3, num_groups=2, device=dev)
    st.update(model, xd, tfd, eid, torch.tensor([1, 0], dtype=torch.int32, device=dev))
    for l in range(2):
        a = attn[l].cpu().numpy()
        _assert_distributions(a, f"N=2911 block {l}")
        _assert_stats(st.node_stats[:, l].cpu().numpy(), st.lag_stats[:, l].cpu().numpy(), st.matrix_stats[:, l].cpu().numpy(),
                      st.counts.cpu().numpy(), a, [1, 0], 2, f"N=2911 block {l} statistics", fast=True)
