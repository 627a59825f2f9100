"""The fp32 step's fused passes around ln_f, the head, the embd dropout, d c_attn and the LayerNorm gamma / beta reductions:
every one of them computes what the separate passes compute, bit for bit.

  A  tecm_layernorm_fwd writes dropout(LN(x)) as an fp32 sequence-major matrix (the head's operand), tecm_layernorm_bwd takes
     the fp32 gradient of that matrix in the same layout and applies the mask itself;
  B  tecm_layernorm_bwd leaves out the store of the unmasked dx when only dropout(dx) has a reader;
  C  d c_attn (+ d z) as an N = 768 launch plus an N = 32 launch instead of one K-extended N = 800 launch;
  D  one native call reduces the partials of several LayerNorm backwards;
  and the whole fp32 model with all four routes against the same step with every switch off.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_cpu as R  # noqa: E402
from tests.parity import build_model, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

D = 768
SWITCHES = ("TECM_FUSE_HEAD", "TECM_EMBD_MASKED_GRAD", "TECM_SPLIT_DCATTN", "TECM_LN_BATCH_REDUCE")
SPATIAL = ("spatio_temporal_embedding.", "spatial_encoder.")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _rand(*shape, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dev)


def _ln_inputs(dev, M):
    x = _rand(M, D, dev=dev, seed=1)
    g, b = 1 + 0.1 * _rand(D, dev=dev, seed=2), 0.1 * _rand(D, dev=dev, seed=3)
    return x, g, b


def _to_seq(tm, B, T, N):
    """time-major rows (b, t, n) -> the (B, N, T*D) matrix with rows (b, n, t)."""
    return tm.view(B, T, N, D).permute(0, 2, 1, 3).reshape(B, N, T * D).contiguous()


def _to_tm(seq, B, T, N):
    return seq.view(B, N, T, D).permute(0, 2, 1, 3).reshape(B * T * N, D).contiguous()


@pytest.mark.parametrize("p", [0.1, 0.0])
@pytest.mark.parametrize("T", [3, 6])
def test_fp32_sequence_major_forward_equals_layernorm_dropout_permute(dev, T, p):
    """B = 2, N = 37 (M = 222 / 444 rows: no multiple of a block's 4 rows at T = 3): layernorm_fwd -> dropout_apply -> permute
    to (b, n, t) on the existing path against the one launch, values and saved statistics."""
    from tecmollm import ops
    B, N = 2, 37
    M = B * T * N
    x, g, b = _ln_inputs(dev, M)
    st, st_r = torch.empty(M, 2, device=dev), torch.empty(M, 2, device=dev)
    spec = ops.drop(p, 777, D) if p > 0 else None
    seq = torch.full((B, N, T * D), float("nan"), device=dev)
    ops.layernorm_fwd(x, D, g, b, None, D, st, M, D, y16d=seq, ldy16d=D, drop16d=spec if spec is not None else ops.NO_DROP,
                      seq_major=(T, N))
    y = torch.empty(M, D, device=dev)
    ops.layernorm_fwd(x, D, g, b, y, D, st_r, M, D)
    yd = ops.dropout_apply(y, M, D, spec) if spec is not None else y
    assert torch.equal(seq, _to_seq(yd, B, T, N))
    assert torch.equal(st, st_r)
    if p > 0:
        assert 0.05 < float((seq == 0).float().mean()) < 0.15


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("with_dres", [True, False])
@pytest.mark.parametrize("p", [0.1, 0.0])
@pytest.mark.parametrize("T", [3, 6])
def test_fp32_sequence_major_gradient_equals_the_unpermuted_masked_one(dev, T, p, with_dres, masked):
    """tecm_layernorm_bwd with TecmLnDyMap and an fp32 dy against the plain kernel fed the un-permuted, masked gradient: dx,
    dx_masked and the reduced dgamma / dbeta."""
    from tecmollm import ops
    B, N = 2, 37
    M = B * T * N
    x, g, b = _ln_inputs(dev, M)
    st = torch.empty(M, 2, device=dev)
    ops.layernorm_fwd(x, D, g, b, torch.empty(M, D, device=dev), D, st, M, D)
    spec = ops.drop(p, 777, D) if p > 0 else None
    dseq = _rand(B, N, T * D, dev=dev, seed=4)
    dres = _rand(M, D, dev=dev, seed=5) if with_dres else None
    mk = dict(mask_drop=ops.drop(0.1, 7, D)) if masked else {}
    dx, dx_r = torch.empty(M, D, device=dev), torch.empty(M, D, device=dev)
    dxm, dxm_r = (torch.empty(M, D, device=dev), torch.empty(M, D, device=dev)) if masked else (None, None)
    dg, db = ops.layernorm_bwd(dseq, D, x, D, g, st, dres, dx, M, D, dx_masked=dxm, dy_seq_major=(T, N, spec),
                               dy_seq_fp32=True, **mk)
    dy_tm = _to_tm(dseq, B, T, N)
    if spec is not None:
        dy_tm = ops.dropout_apply(dy_tm, M, D, spec)
    dg_r, db_r = ops.layernorm_bwd(dy_tm, D, x, D, g, st, dres, dx_r, M, D, dx_masked=dxm_r, **mk)
    assert torch.equal(dx, dx_r) and torch.equal(dg, dg_r) and torch.equal(db, db_r)
    if masked:
        assert torch.equal(dxm, dxm_r)


@pytest.mark.parametrize("M", [222, 4099])
def test_skip_dx_leaves_the_dx_buffer_alone_and_the_masked_gradient_unchanged(dev, M):
    from tecmollm import ops
    x, g, b = _ln_inputs(dev, M)
    st = torch.empty(M, 2, device=dev)
    ops.layernorm_fwd(x, D, g, b, torch.empty(M, D, device=dev), D, st, M, D)
    dy, dres, dy2 = _rand(M, D, dev=dev, seed=4), _rand(M, D, dev=dev, seed=5), _rand(M, D, dev=dev, seed=6)
    add = (dy2, D, ops.drop(0.1, 5, 800))
    dx_r, dxm_r = torch.empty(M, D, device=dev), torch.empty(M, D, device=dev)
    dg_r, db_r = ops.layernorm_bwd(dy, D, x, D, g, st, dres, dx_r, M, D, dx_masked=dxm_r, mask_drop=ops.drop(0.1, 7, D), add=add)
    dx = torch.full((M, D), -12345.0, device=dev)
    dxm = torch.empty(M, D, device=dev)
    dg, db = ops.layernorm_bwd(dy, D, x, D, g, st, dres, dx, M, D, dx_masked=dxm, mask_drop=ops.drop(0.1, 7, D), add=add,
                               skip_dx=True)
    assert torch.equal(dxm, dxm_r) and torch.equal(dg, dg_r) and torch.equal(db, db_r)
    assert bool((dx == -12345.0).all())
    assert not torch.equal(dxm_r, dx_r)                                    # the mask did something
    with pytest.raises(ops._lib.TecmError):                                # nothing would be written at all
        ops.layernorm_bwd(dy, D, x, D, g, st, dres, dx, M, D, skip_dx=True)


def test_d_c_attn_as_a_768_and_a_32_column_launch_equals_the_one_launch(dev):
    """M = 300 (no multiple of the 128-row tile), KE = 800, F3 = 2304: du from the split pair against the K-extended launch."""
    from tecmollm import ops
    M, KE, F3, R_ = 300, 800, 2304, 32
    dqkv = _rand(M, F3, dev=dev, seed=1)
    wcat = 0.05 * _rand(KE, F3, dev=dev, seed=2)
    du_r = torch.empty(M, KE, device=dev)
    ops.gemm(M, KE, F3, dqkv, F3, wcat, F3, du_r, KE)
    du = torch.full((M, KE), float("nan"), device=dev)
    ops.gemm(M, D, F3, dqkv, F3, wcat, F3, du, KE)
    ops.gemm(M, R_, F3, dqkv, F3, wcat, F3, du, KE, b_off=D * F3, c_off=D)
    assert torch.equal(du, du_r)
    assert rel_err(du.cpu(), dqkv.cpu().double() @ wcat.cpu().double().t()) < 1e-5


@pytest.mark.parametrize("M", [300, 5000])
def test_batched_reduction_equals_one_colsum_per_buffer(dev, M):
    """Three partials buffers of layernorm_bwd_blocks(M, 768) rows (75 and 1024): one call against three colsum calls."""
    from tecmollm import ops
    nb = ops.layernorm_bwd_blocks(M, D)
    assert nb == min(1024, (M + 3) // 4)
    mats = [_rand(nb, 2 * D, dev=dev, seed=10 + i) * (10.0 ** i) for i in range(3)]
    got = ops.colsum_batch(mats, nb, 2 * D)
    for i, m in enumerate(mats):
        want = ops.colsum(m, 2 * D, nb, 1, 1, 2 * D)
        assert torch.equal(got[i], want[0]), i
    assert rel_err(got[0].cpu(), mats[0].cpu().double().sum(0)) < 1e-5


# ------------------------------------------------------------------------------------------------ whole model
def _model_step(model, x, tf, ei, y, off, monkeypatch):
    """One forward + Huber + backward with fixed dropout masks; off: every route of this file switched off."""
    from src.model import modules as M_
    from tecmollm import memory, ops
    for k in SWITCHES:
        if off:
            monkeypatch.setenv(k, "0")
        else:
            monkeypatch.delenv(k, raising=False)
    memory.clear_choices()
    model.zero_grad(set_to_none=True)
    torch.manual_seed(11)
    M_._seed_counter[0] = 0
    out = model(x, tf, ei)
    loss, dout = ops.huber_fwd_bwd_strided(out.detach(), y, 1.0, 1.0)
    out.backward(dout)
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    return loss.clone(), grads


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("L_in", [48, 96])
def test_whole_fp32_model_with_the_new_routes_equals_the_separate_passes(dev, L_in, train, monkeypatch):
    """fp32, N = 135 (9 x 15 grid), B = 2, T = L_in / 16: loss and all 66 gradients of a train-mode (p = 0.1) and an
    eval-mode step, new routes against TECM_FUSE_HEAD=0 + the other three switches off, torch.equal.  The spatial stage
    accumulates its 11 parameter gradients with float atomics, which can move their last bits between two runs of the SAME
    code: where two runs of the switched-off step differ from each other in such a tensor, that tensor alone is held to
    the bar tests/test_gpu_recompute.py uses for this case instead (every other tensor stays torch.equal)."""
    N, B = 135, 2
    cfg = R.default_config(L_in=L_in, L_out=12, num_nodes=N, c_in=10, d_emb=12)
    model = build_model(cfg, R.init_params(cfg, seed=3), "cuda", "per_timestep", precision="fp32").train(train)
    x, tf, y = R.synthetic_batch(B, L_in, N, 10, 12, seed=4)
    tfd = tf[:, :, 0, :].contiguous().cuda().unsqueeze(-2).expand(B, L_in, N, 4)
    ei = R.grid_graph(9, 15, threshold_km=150.0)[0].cuda()
    x, y = x.cuda(), y.cuda()
    l_off, g_off = _model_step(model, x, tf=tfd, ei=ei, y=y, off=True, monkeypatch=monkeypatch)
    _, g_off2 = _model_step(model, x, tf=tfd, ei=ei, y=y, off=True, monkeypatch=monkeypatch)
    l_on, g_on = _model_step(model, x, tf=tfd, ei=ei, y=y, off=False, monkeypatch=monkeypatch)
    assert len(g_off) == 66 and g_on.keys() == g_off.keys()
    assert torch.equal(l_on, l_off)
    wobbly = [k for k in g_off if not torch.equal(g_off[k], g_off2[k])]
    assert all(k.startswith(SPATIAL) for k in wobbly), wobbly
    print(f"L_in={L_in} train={train}: tensors that differ between two switched-off runs: {wobbly}")
    for k in g_off:
        if k in wobbly:
            d = (g_on[k] - g_off[k]).abs()
            rms = g_off[k].pow(2).mean().sqrt()
            assert rel_err(g_on[k], g_off[k]) <= 1e-5 and bool((d <= 1e-4 * g_off[k].abs() + 1e-5 * rms).all()), k
        else:
            assert torch.equal(g_on[k], g_off[k]), k
