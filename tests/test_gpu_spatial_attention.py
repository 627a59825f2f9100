"""GPU tests of the spatial attention maps (csrc/spatial_attn.hip through tecmollm/spatial_attention.py): the exported
coefficients against the float64 restatement of GATv2 (tests/spatial_attention_ref.py, tied to the frozen oracle by
tests/test_host_spatial_attention.py), on hard rows, as distributions, against the production forward, across workspace
chunks, through `SpatialEncoder.forward(return_attention_weights=True)`, the fp64 accumulator and its groups,
`evaluate_attention`, a bad time index and the full 41 x 71 grid.

Bars.  alpha: |kernel - float64| <= parity.RTOL * |float64| + 1e-12 (an fp32 restatement of the same algorithm on the CPU
differs from float64 by 5e-7 relative at N(0, 1) inputs, 1.2e-5 with `att` scaled by 20, 1.7e-5 with `att` x 10 and x x 4).
A row sums to 1 within (deg + 1) * 2^-23: the denominator is the fp32 sum of exactly the deg + 1 terms that are divided, so
the sum of the quotients is off by at most (deg + 2) * 2^-24.  sum alpha and sum alpha^2 are bit-exact against a numpy
float64 loop over the exported fp32 alpha in ascending graph order (the square of an fp32 value is exact in float64); sum m
and sum entropy within 1e-6 relative of the same loop fed with float64 values formed from the exported alpha."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import parity
from tests import spatial_attention_ref as A

pytestmark = pytest.mark.gpu

B, L, N = 2, 3, 20
_models = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _model(dev, c_in=6, num_nodes=N, mode="per_timestep"):
    """(model in eval mode, oracle parameter dict); one GPT-2 block: only the spatial stage is looked at."""
    key = (c_in, num_nodes)
    if key not in _models:
        cfg = R.default_config(L_in=16, L_out=12, num_nodes=num_nodes, c_in=c_in, d_emb=22 - c_in, llm_layers=1)
        params = R.init_params(cfg, seed=11 + c_in)
        _models[key] = (parity.build_model(cfg, params, dev, mode).eval(), params)
    model, params = _models[key]
    model.gat_graphs = model.spatial_encoder.gat_graphs = mode
    return model, params


def _inputs(c_in=6, num_nodes=N, per_node=False, b=B, l=L, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(b, l, num_nodes, c_in, generator=g)
    shape = (b, l, num_nodes) if per_node else (b, l, 1)
    tf = torch.stack([torch.randint(0, hi, shape, generator=g) for hi in (12, 366, 13, 4)], -1).float()
    return x, tf.expand(b, l, num_nodes, 4)


def _assert_alpha(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    worst = float(np.max(err / (parity.RTOL * np.abs(want) + 1e-12)))
    print(f"{what}: max |kernel - float64| / (RTOL |float64| + 1e-12) = {worst:.3e}; max relative error "
          f"{float(np.max(err / np.maximum(np.abs(want), 1e-300))):.3e}")
    assert worst <= 1.0, (what, worst)


EI = A.irregular_graph(N)


@pytest.mark.parametrize("c_in", [6, 10])
@pytest.mark.parametrize("per_node", [False, True])
@pytest.mark.parametrize("mode", ["per_timestep", "reference"])
def test_alpha_matches_the_float64_reference(dev, c_in, per_node, mode):
    from tecmollm import check_device_errors, spatial_attention
    model, params = _model(dev, c_in, mode=mode)
    x, tf = _inputs(c_in, per_node=per_node, seed=c_in)
    ei_sl, alpha = spatial_attention(model, x.to(dev), tf.to(dev), EI.to(dev))
    want, _, _, _ = A.model_attention(x, tf, EI.numpy(), params, B * L if mode == "per_timestep" else 1)
    E2 = want.shape[2]
    assert alpha.is_cuda and alpha.dtype == torch.float32 and alpha.shape == (B, L, E2, 2)
    assert ei_sl.dtype == torch.int64 and ei_sl.cpu().numpy().tolist() == A.edge_index_sl(EI.numpy(), N).tolist()
    _assert_alpha(alpha.cpu().numpy(), want, f"alpha c_in={c_in} per_node={per_node} {mode}")
    check_device_errors(dev)
    model.train()                                    # pre-dropout coefficients under any training flag
    try:
        assert torch.equal(spatial_attention(model, x.to(dev), tf.to(dev), EI.to(dev))[1], alpha)
    finally:
        model.eval()


def test_hard_rows(dev):
    """att x 20: a logit spread of ~50 inside a row, smallest alpha ~1e-22, same bar.  att x 10 and x x 4: spread ~175, fp32
    underflows to exact zeros: every alpha finite, entries >= 1e-6 inside the bar, smaller ones below 2e-6, the argmax entry of
    every (target, head) the reference's."""
    from tecmollm import spatial_attention
    model, params = _model(dev, 6)
    x, tf = _inputs(6, seed=3)
    p20 = dict(params)
    p20[R.P_GAT + "att"] = params[R.P_GAT + "att"] * 20
    att0 = model.spatial_encoder.gat_conv.att.detach().clone()
    try:
        with torch.no_grad():
            model.spatial_encoder.gat_conv.att.copy_((params[R.P_GAT + "att"] * 20).to(dev))
        alpha = spatial_attention(model, x.to(dev), tf.to(dev), EI.to(dev))[1].cpu().numpy()
        want = A.model_attention(x, tf, EI.numpy(), p20, B * L)[0]
        pos = want[want > 0]
        print(f"att x 20: smallest reference alpha {pos.min():.3e}")
        _assert_alpha(alpha, want, "att x 20")
        p10 = dict(params)
        p10[R.P_GAT + "att"] = params[R.P_GAT + "att"] * 10
        with torch.no_grad():
            model.spatial_encoder.gat_conv.att.copy_((params[R.P_GAT + "att"] * 10).to(dev))
        x4 = x * 4
        alpha = spatial_attention(model, x4.to(dev), tf.to(dev), EI.to(dev))[1].cpu().numpy()
        want = A.model_attention(x4, tf, EI.numpy(), p10, B * L)[0]
    finally:
        with torch.no_grad():
            model.spatial_encoder.gat_conv.att.copy_(att0)
    assert np.isfinite(alpha).all()
    big = want >= 1e-6
    _assert_alpha(alpha[big], want[big], "att x 10, x x 4, reference >= 1e-6")
    print(f"att x 10, x x 4: largest kernel alpha where the reference is below 1e-6: {alpha[~big].max():.3e}; "
          f"exact zeros: {int((alpha == 0).sum())}")
    assert (alpha[~big] < 2e-6).all()
    dst = A.edge_index_sl(EI.numpy(), N)[1]
    for i in range(N):
        rows = np.nonzero(dst == i)[0]
        assert (alpha[:, :, rows].argmax(axis=2) == want[:, :, rows].argmax(axis=2)).all(), i


def test_rows_are_distributions(dev):
    from tecmollm import AttentionStats, spatial_attention
    ei_sl = A.edge_index_sl(EI.numpy(), N)
    dst = ei_sl[1]
    deg = np.bincount(dst[:-N], minlength=N)
    assert deg[7] == 0 and deg.max() >= 9
    for mode in ("per_timestep", "reference"):
        model, _ = _model(dev, 6, mode=mode)
        x, tf = _inputs(6, seed=4)
        alpha = spatial_attention(model, x.to(dev), tf.to(dev), EI.to(dev))[1].cpu().numpy()
        sums = np.zeros((B, L, N, 2))
        for e in range(dst.size):
            sums[:, :, dst[e]] += alpha[:, :, e].astype(np.float64)
        connected = np.array([[t * B + b < (B * L if mode == "per_timestep" else 1) for t in range(L)] for b in range(B)])
        bound = np.where(connected[:, :, None, None], (deg + 1.0)[None, None, :, None], 1.0) * 2.0 ** -23
        print(f"{mode}: max |row sum - 1| / ((deg + 1) 2^-23) = {float(np.max(np.abs(sums - 1.0) / bound)):.3f}")
        assert (np.abs(sums - 1.0) <= bound).all()
        lone = ~connected
        assert (alpha[lone][:, -N:] == 1.0).all() and (alpha[lone][:, :-N] == 0.0).all()
        if mode == "reference":                      # entropy of the unconnected graphs: exactly 0 (they go to group 1)
            st = AttentionStats(N, dst.size, 2, device=dev)
            ids = torch.ones(B, L, dtype=torch.int32)
            ids[0, 0] = 0
            st.update(model, x.to(dev), tf.to(dev), EI.to(dev), ids.to(dev), skip_unconnected=False)
            assert st.counts.tolist() == [1, B * L - 1]
            assert (st.node_stats[1] == 0).all() and (st.node_stats[0].cpu().numpy()[deg > 0] > 0).all()
            assert (st.edge_stats[1, 0, -N:] == B * L - 1).all() and (st.edge_stats[1, 0, :-N] == 0).all()


def _forward_agreement(dev, model, x, tf, ei, what):
    """Eval-mode SpatialFn output minus h minus bias against sum_j alpha_ij x_l[j], x_l formed by torch on the device."""
    from tecmollm import functions as F_
    from tecmollm import graph as graph_
    from tecmollm import spatial_attention
    b, l, n, c_in = x.shape
    x, tf, ei = x.to(dev), tf.to(dev), ei.to(dev)
    emb, enc = model.spatio_temporal_embedding, model.spatial_encoder
    with torch.no_grad():
        meta = graph_.get(ei, n, dev, emb.d_emb)
        R_ = 1 if model.gat_graphs == "reference" else b * l
        plan = F_.DropPlan(training=False, p=0.0, base_seed=0)
        out = F_.SpatialFn.apply(x, tf, *emb.tables(), *enc.params(), meta, model.heads, R_, plan)[..., :22]
        node, tod, doy, year, season = emb.tables()
        idx = tf.long()
        temporal = ((tod[idx[..., 0]] + doy[idx[..., 1]]) + year[idx[..., 2]]) + season[idx[..., 3]]
        h = torch.cat([x, node.view(1, 1, n, -1) + temporal], -1)
        Wl, bl, _, _, _, bias = enc.params()
        xl = (h @ Wl.t() + bl).view(b, l, n, 2, 11)
        ei_sl, alpha = spatial_attention(model, x, tf, ei)
        agg = torch.zeros(b, l, n, 2, 11, device=dev)
        agg.index_add_(2, ei_sl[1], alpha.unsqueeze(-1) * xl[:, :, ei_sl[0]])
        want = (out - h - bias).double()
        got = agg.view(b, l, n, 22).double()
        rms = float(out.double().pow(2).mean().sqrt())
        worst = float(((got - want).abs() / (parity.RTOL * want.abs() + parity.ATOL_RMS * rms)).max())
    print(f"{what}: max |sum alpha x_l - (out - h - bias)| / (RTOL |.| + ATOL_RMS rms(out)) = {worst:.3e}")
    assert worst <= 1.0, (what, worst)
    return ei_sl, alpha


def banded_graph(num_nodes, band=12, per_node=6, seed=2):
    """Edges j -> i with 0 < |j - i| <= band, about `per_node` per target, in random order."""
    rng = np.random.default_rng(seed)
    edges = []
    for i in range(num_nodes):
        for _ in range(per_node):
            j = i + int(rng.integers(-band, band + 1))
            if 0 <= j < num_nodes and j != i:
                edges.append((j, i))
    order = rng.permutation(len(edges))
    return torch.tensor([edges[k] for k in order], dtype=torch.int64).t().contiguous()


@pytest.mark.parametrize("num_nodes", [20, 300])
def test_agrees_with_the_production_forward(dev, num_nodes):
    """N = 300: the rows of one graph span block boundaries, and the forward's default tiling has several tiles."""
    from tecmollm import graph as graph_
    ei = EI if num_nodes == 20 else banded_graph(300)
    for mode in ("per_timestep", "reference"):
        model, _ = _model(dev, 6, num_nodes, mode)
        x, tf = _inputs(6, num_nodes, seed=5)
        _forward_agreement(dev, model, x, tf, ei, f"N={num_nodes} {mode}")
    if num_nodes == 300:
        assert graph_.get(ei.to(dev), 300, dev, 16).num_tiles > 1


def _stats(dev, model, batches, ei, G=1, ids=None, skip=False, max_ws_bytes=None):
    from tecmollm import AttentionStats
    n = batches[0][0].shape[2]
    st = AttentionStats(n, A.edge_index_sl(ei.numpy(), n).shape[1], G, device=dev)
    for k, (x, tf) in enumerate(batches):
        st.update(model, x.to(dev), tf.to(dev), ei.to(dev), None if ids is None else ids[k].to(dev), skip,
                  max_ws_bytes=max_ws_bytes)
    return st


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in ((a.edge_stats, b.edge_stats), (a.node_stats, b.node_stats), (a.counts, b.counts)))


def test_chunking_changes_no_bit(dev):
    from tecmollm import ops, spatial_attention
    from tecmollm.spatial_attention import _model_descriptor
    model, _ = _model(dev, 6)
    x, tf = _inputs(6, seed=6)
    eid = EI.to(dev)
    d, meta, keep = _model_descriptor(model, x.to(dev), tf.to(dev), eid)
    whole = spatial_attention(model, x.to(dev), tf.to(dev), eid)[1]
    st = _stats(dev, model, [(x, tf)], EI, G=2, ids=[torch.tensor([[0, 1, 0], [1, 1, 0]], dtype=torch.int32)])
    for accumulate, graphs_per_chunk in ((False, 2), (False, 1), (True, 2), (True, 1)):
        per_graph = ops.spatial_attention_ws_floats(d, meta.num_edges, accumulate) // (B * L)
        assert per_graph * B * L == ops.spatial_attention_ws_floats(d, meta.num_edges, accumulate)   # one chunk by default
        cap = 4 * per_graph * graphs_per_chunk + 4 * (per_graph // 2)        # not a whole number of graphs: >= 3 chunks
        if accumulate:
            got = _stats(dev, model, [(x, tf)], EI, G=2, ids=[torch.tensor([[0, 1, 0], [1, 1, 0]], dtype=torch.int32)],
                         max_ws_bytes=cap)
            assert _same_bits(got, st)
        else:
            assert torch.equal(spatial_attention(model, x.to(dev), tf.to(dev), eid, max_ws_bytes=cap)[1], whole)
    from tecmollm import TecmError
    with pytest.raises(TecmError):                   # a workspace that does not hold one graph is refused, not shrunk into
        spatial_attention(model, x.to(dev), tf.to(dev), eid, max_ws_bytes=4 * (per_graph // 4))
    del keep


@pytest.mark.parametrize("mode", ["per_timestep", "reference"])
def test_return_attention_weights_on_the_stand_alone_encoder(dev, mode):
    from src.model.modules import SpatialEncoder
    cfg = R.default_config(num_nodes=N)
    p = R.init_params(cfg, seed=6)
    enc = SpatialEncoder(22, 11, 2).eval()
    enc.load_state_dict({k[len("spatial_encoder."):]: v for k, v in p.items() if k.startswith(R.P_GAT)})
    enc = enc.to(dev)
    enc.gat_graphs = mode
    G = 4
    x = torch.randn(G, N, 22, generator=torch.Generator().manual_seed(7))
    plain = enc(x.to(dev), EI.to(dev))
    out, (ei_sl, alpha) = enc(x.to(dev), EI.to(dev), return_attention_weights=True)
    assert torch.equal(out, plain) and torch.equal(enc(x.to(dev), EI.to(dev), None, False), plain)
    assert ei_sl.cpu().numpy().tolist() == A.edge_index_sl(EI.numpy(), N).tolist()
    want = np.stack([A.gat_attention(x[g].numpy(), EI.numpy(), p, mode == "per_timestep" or g == 0)[0] for g in range(G)])
    assert alpha.shape == (G, want.shape[1], 2)
    _assert_alpha(alpha.cpu().numpy(), want, f"stand-alone encoder, {mode}")


def test_accumulator_sums(dev):
    """Two batches into one group: reproducible bits; sum alpha and sum alpha^2 bit for bit the ordered float64 loop over the
    exported alpha; sum m and sum entropy within 1e-6 relative of the loop fed with float64 values from the exported alpha."""
    from tecmollm import spatial_attention
    model, params = _model(dev, 6)
    batches = [_inputs(6, seed=7), _inputs(6, seed=8)]
    st = _stats(dev, model, batches, EI)
    assert _same_bits(st, _stats(dev, model, batches, EI))
    ei_sl = A.edge_index_sl(EI.numpy(), N)
    stats = None
    for x, tf in batches:
        alpha = spatial_attention(model, x.to(dev), tf.to(dev), EI.to(dev))[1].cpu().numpy().reshape(B * L, -1, 2)
        xl = A.model_attention(x, tf, EI.numpy(), params, B * L)[1].reshape(B * L, N, 2, 11)
        msg = alpha.astype(np.float64) * np.linalg.norm(xl, axis=-1)[:, ei_sl[0]]
        ent = np.stack([A.entropy_of(a, ei_sl[1], N) for a in alpha])
        stats = A.accumulate_ref(alpha, msg, ent, None, 1, stats)
    edge, node, counts = stats
    got = st.edge_stats_pyg().cpu().numpy()
    assert st.counts.tolist() == counts.tolist() == [2 * B * L]
    assert np.array_equal(got[:, 0], edge[:, 0]) and np.array_equal(got[:, 1], edge[:, 1])
    for name, g, w in (("sum m", got[:, 2], edge[:, 2]), ("sum entropy", st.node_stats.cpu().numpy(), node)):
        rel = np.abs(g - w) / np.where(w == 0, 1.0, np.abs(w))
        print(f"{name}: max relative error {float(rel.max()):.3e}")
        assert (np.abs(g - w) <= 1e-6 * np.abs(w)).all(), name
    # compute() is derive() of these sums, in PyG's order
    out = st.compute()
    want = A.derive_ref(got, st.node_stats.cpu().numpy(), st.counts.cpu().numpy(), ei_sl, N)
    for k, v in want.items():
        np.testing.assert_allclose(out[k], v, rtol=1e-14, atol=0, err_msg=k)


def test_groups_and_bad_ids(dev):
    """G = 3 with ids mixed inside the batch: every group's sums are the single-group sums of its own graphs, fed one graph at a
    time in ascending order.  An id of 3 or -1 skips its graph, leaves the other groups' bits alone and raises at the boundary."""
    from tecmollm import TecmError, check_device_errors
    model, _ = _model(dev, 6)
    x, tf = _inputs(6, seed=9)
    ids = torch.tensor([[0, 2, 1], [1, 2, 0]], dtype=torch.int32)           # graph (b, t) -> group
    st = _stats(dev, model, [(x, tf)], EI, G=3, ids=[ids])
    check_device_errors(dev)
    assert st.counts.tolist() == [2, 2, 2]

    def own(keep):                                                          # one single-graph update per kept graph, gm ascending
        graphs = [(x[b:b + 1, t:t + 1], tf[b:b + 1, t:t + 1]) for b in range(B) for t in range(L) if keep(b, t)]
        return _stats(dev, model, graphs, EI)
    for g in range(3):
        one = own(lambda b, t: int(ids[b, t]) == g)
        assert torch.equal(one.edge_stats[0], st.edge_stats[g]) and torch.equal(one.node_stats[0], st.node_stats[g]), g
    bad = ids.clone()
    bad[0, 1], bad[1, 1] = 3, -1                                            # both graphs of group 2
    sb = _stats(dev, model, [(x, tf)], EI, G=3, ids=[bad])
    assert sb.counts.tolist() == [2, 2, 0]
    for g in (0, 1):
        assert torch.equal(sb.edge_stats[g], st.edge_stats[g]) and torch.equal(sb.node_stats[g], st.node_stats[g])
    assert not sb.edge_stats[2].any() and not sb.node_stats[2].any()
    with pytest.raises(TecmError, match="TECM_BAD_GROUP"):
        check_device_errors(dev)
    check_device_errors(dev)                                                # reported once
    assert np.isnan(sb.compute()["mean"][2]).all()


def test_skip_unconnected_counts_in_reference_mode(dev):
    model, _ = _model(dev, 6, mode="reference")
    batches = [_inputs(6, seed=10), _inputs(6, seed=11)]
    on = _stats(dev, model, batches, EI, skip=True)
    off = _stats(dev, model, batches, EI, skip=False)
    assert on.counts.tolist() == [2] and off.counts.tolist() == [2 * B * L]
    first = [(x[:1, :1], tf[:1, :1]) for x, tf in batches]                  # graph (b = 0, t = 0) of every call
    assert _same_bits(on, _stats(dev, _model(dev, 6, mode="per_timestep")[0], first, EI))
    model, _ = _model(dev, 6, mode="per_timestep")
    assert _stats(dev, model, batches, EI, skip=True).counts.tolist() == [2 * B * L]


class _Windows:
    """A device-resident data set of synthetic windows (tecmollm.synthetic.synthetic_batch) with the `batch` interface the
    evaluation loops read."""

    def __init__(self, S, l, n, c_in, dev):
        from tecmollm.synthetic import synthetic_batch
        x, tf, y = synthetic_batch(S, l, n, c_in, 12, seed=21)
        self.x, self.tf, self.y = x.to(dev), tf.contiguous().to(dev), y.to(dev)

    def __len__(self):
        return self.x.shape[0]

    def batch(self, chunk):
        idx = torch.as_tensor(chunk, dtype=torch.int64, device=self.x.device)
        return self.x[idx], self.tf[idx], self.y[idx]


def test_evaluate_attention_is_the_loop_of_updates(dev):
    from tecmollm import (AttentionStats, evaluate_attention, graph_groups_by_lag, graph_groups_by_sample,
                          graph_groups_by_slot)
    model, _ = _model(dev, 6)
    S, l = 7, 4
    ds = _Windows(S, l, N, 6, dev)
    eid = EI.to(dev)
    E2 = A.edge_index_sl(EI.numpy(), N).shape[1]
    # the helpers
    slot = graph_groups_by_slot(ds.tf)
    assert slot.is_cuda and slot.dtype == torch.int32 and torch.equal(slot, ds.tf[:, :, 0, 0].to(torch.int32))
    lag = graph_groups_by_lag(3, l, dev)
    assert lag.dtype == torch.int32 and lag.tolist() == [list(range(l))] * 3
    kp = torch.tensor([0, 2, 1, 1, 0, 2, 2], dtype=torch.int32, device=dev)
    assert graph_groups_by_sample(kp[:2], l).tolist() == [[0] * l, [2] * l]
    for groups, G, make in ((None, 1, lambda idx, tf: None), ("slot", 12, lambda idx, tf: graph_groups_by_slot(tf)),
                            ("lag", l, lambda idx, tf: graph_groups_by_lag(len(idx), l, dev)),
                            (kp, 3, lambda idx, tf: graph_groups_by_sample(kp[idx], l))):
        got = evaluate_attention(model, ds, eid, 3, groups=groups, num_groups=G if groups is kp else None)
        st = AttentionStats(N, E2, G, device=dev)
        for a in range(0, S, 3):
            idx = list(range(a, min(S, a + 3)))
            x, tf, _ = ds.batch(idx)
            st.update(model, x, tf, eid, make(idx, tf))
        want = st.compute()
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(got[k], want[k], equal_nan=True), (groups, k)
        assert got["count"].sum() == S * l
    assert evaluate_attention(model, ds, eid, 3, groups="lag")["count"].tolist() == [S] * l
    host = ds.tf[:, :, 0, 0].cpu().numpy().astype(int).reshape(-1).tolist()
    assert evaluate_attention(model, ds, eid, 3, groups="slot")["count"].tolist() == [host.count(s) for s in range(12)]
    from tecmollm import TecmError
    with pytest.raises(TecmError, match="TECM_BAD_GROUP"):
        evaluate_attention(model, ds, eid, 3, groups=kp, num_groups=2)


def test_bad_time_index_gives_nan_rows_and_sets_the_flag(dev):
    from tecmollm import check_device_errors, devcheck, spatial_attention
    model, _ = _model(dev, 6)
    x, tf = _inputs(6, seed=12)
    tf = tf.clone()
    tf[1, 2, :, 1] = 400.0                                                  # day-of-year outside [0, 366) in graph (b = 1, t = 2)
    check_device_errors(dev)
    alpha = spatial_attention(model, x.to(dev), tf.to(dev), EI.to(dev))[1]
    torch.cuda.synchronize()
    assert int(devcheck.error_word(dev).word.item()) == devcheck.BAD_DOY
    a = alpha.cpu().numpy()
    assert np.isnan(a[1, 2]).all()
    a[1, 2] = 0
    assert np.isfinite(a).all()
    with pytest.raises(IndexError, match="day-of-year"):
        check_device_errors(dev)


def test_full_grid(dev):
    """N = 2911 on the 41 x 71 grid, B = 1, L = 4, every timestep a graph: rows sum to 1, and the coefficients reproduce the
    production forward's aggregation."""
    from tecmollm.synthetic import grid_graph
    ei = grid_graph()[0]
    n = 2911
    model, _ = _model(dev, 6, n, "per_timestep")
    x, tf = _inputs(6, n, b=1, l=4, seed=13)
    ei_sl, alpha = _forward_agreement(dev, model, x, tf, ei, "N=2911")
    dst = ei_sl[1]
    deg = torch.bincount(dst[:-n], minlength=n).double()
    sums = torch.zeros(1, 4, n, 2, dtype=torch.float64, device=dev).index_add_(2, dst, alpha.double())
    ratio = float(((sums - 1).abs() / ((deg + 1).view(1, 1, n, 1) * 2.0 ** -23)).max())
    print(f"N=2911: max |row sum - 1| / ((deg + 1) 2^-23) = {ratio:.3f}; in-degree up to {int(deg.max())}")
    assert ratio <= 1.0
