"""bf16 mode (BASELINE configs[2] = the reference's own training arithmetic, train.py:68), model level, forward AND
backward, against the bf16-EMULATING oracle: oracle/ref_cpu.py `Rounding` / `_MatMul` / `_Conv1d` apply the same bf16
operand roundings to the forward and to both backward contractions of every Linear / Conv1d the HIP path runs on the
bf16 matrix cores (and leave exact the ones it runs on the fp32 kernel).

Three layers of evidence, tightest first (bars and their justification: tests/parity.py):
  1. every STAGE (conv block, patch projection, one GPT-2 block, head) with identical inputs and identical upstream
     gradients on both sides: 1e-2 element-wise for the output, the input gradient and every parameter gradient;
  2. the whole step (eval and train mode with mirrored masks, N = 20 / 135 / 2911, 3 and 6 tokens), all 66 gradients, at
     the model-level bars -- bf16 roundings amplify ANY deviation to the bf16 noise floor within a few chained stages;
  3. the self-calibrated form of 2: the device is as close to the oracle as the oracle is to itself under a 1e-6
     perturbation of its inputs (the size of the fp32-mode deviation between the two implementations)."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests.parity import (ATOL_RMS_BF16, RTOL_BF16, assert_batch_equals_mean_of_samples, assert_close, assert_parity,
                          batch_vs_single_sample_grads, build_model, compare_forward_backward, device_rounding, l2_rel,
                          oracle_step, rel_err)

pytestmark = pytest.mark.gpu
BF16 = 1                      # tecmollm.ops.PREC_BF16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _close16(a, b, what, atol_rms=ATOL_RMS_BF16):
    assert_close(a, b, what, RTOL_BF16, atol_rms)


def _tm(t, B, N):
    """oracle (S = B*N, T, D) -> device time-major (B, T, N, D)."""
    S, T, D = t.shape
    return t.reshape(B, N, T, D).permute(0, 2, 1, 3).contiguous()


def _seq(t):
    """device (B, T, N, D) -> oracle (S, T, D)."""
    B, T, N, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, T, D)


def _leaf(p, prefix):
    return {k: v.clone().requires_grad_(True) for k, v in p.items() if k.startswith(prefix)}


# ----------------------------------------------------------------------------------- 1. stages, identical inputs
@pytest.mark.parametrize("idx,L,cin,ld", [(0, 48, 22, 24), (1, 24, 64, 64)], ids=["block0", "block1"])
def test_bf16_conv_block_stage_fwd_bwd(dev, idx, L, cin, ld):
    """Multi_Scale_Conv_Block (modules.py:43-60) in bf16 mode: output, d input and the 14 parameter gradients."""
    from src.model.modules import Multi_Scale_Conv_Block
    B, N = 2, 37
    cfg = R.default_config(L_in=48, num_nodes=N)
    p = R.init_params(cfg, seed=41)
    pre = f"{R.P_CONV}{idx}."
    g = torch.Generator().manual_seed(42 + idx)
    x = torch.randn(B * N, L, cin, generator=g)                           # oracle layout (S, L, C)
    pr = _leaf(p, pre)
    xr = x.clone().requires_grad_(True)
    ref = R.conv_block(xr.permute(0, 2, 1), pr, idx, 2, device_rounding(N)).permute(0, 2, 1)       # (S, L/2, Cout)
    gout = torch.randn(ref.shape, generator=g)
    gref = torch.autograd.grad(ref, [xr] + list(pr.values()), gout)

    cout = ref.shape[-1]
    blk = Multi_Scale_Conv_Block(cin, cout, 2)
    blk.load_state_dict({k[len(pre):]: v for k, v in p.items() if k.startswith(pre)})
    blk = blk.to(dev)
    xd = torch.zeros(B, L, N, ld)
    xd[..., :cin] = _tm(x, B, N)
    xd = xd.to(dev).requires_grad_(True)
    out, out16 = blk.forward_tm(xd, cin, True, BF16, None)
    assert out16 is not None and out16.dtype == torch.bfloat16 and torch.equal(out16.float(), out.bfloat16().float())
    _close16(_seq(out), ref, f"conv block {idx} forward")
    named = dict(blk.named_parameters())
    ghip = torch.autograd.grad(out, [xd] + [named[k[len(pre):]] for k in pr], _tm(gout, B, N).to(dev))
    _close16(_seq(ghip[0][..., :cin]), gref[0], f"conv block {idx} d input")
    for k, a, b in zip(pr, ghip[1:], gref[1:]):
        _close16(a, b, k)


def test_bf16_patch_projection_stage_fwd_bwd(dev):
    """LatentPatchingProjection (modules.py:100-119) + wpe in bf16 mode."""
    from src.model.modules import LatentPatchingProjection
    B, N, Lc, D = 2, 33, 12, 128
    cfg = R.default_config(L_in=48, num_nodes=N)
    p = R.init_params(cfg, seed=43)
    g = torch.Generator().manual_seed(44)
    conv = torch.randn(B * N, Lc, D, generator=g)
    W = p[R.P_PATCH + "weight"].clone().requires_grad_(True)
    b = p[R.P_PATCH + "bias"].clone().requires_grad_(True)
    wpe = p[R.P_GPT + "wpe.weight"].clone().requires_grad_(True)
    cr = conv.clone().requires_grad_(True)
    ref = R.mm(cr.reshape(B * N, Lc // 4, 4 * D), W.t(), R.BF16) + b + wpe[:Lc // 4]
    gout = torch.randn(ref.shape, generator=g)
    gref = torch.autograd.grad(ref, [cr, W, b, wpe], gout)
    pj = LatentPatchingProjection(D, 4, 768)
    pj.projection.load_state_dict({"weight": W.detach(), "bias": b.detach()})
    pj = pj.to(dev)
    from tecmollm import functions as F_
    cd = _tm(conv, B, N).to(dev).requires_grad_(True)
    wd = wpe.detach().to(dev).requires_grad_(True)
    out = pj.forward_tm(cd, wd, F_.DropPlan(False, 0.0, 0, BF16), None)
    _close16(_seq(out), ref, "tokens")
    ghip = torch.autograd.grad(out, [cd, pj.projection.weight, pj.projection.bias, wd], _tm(gout, B, N).to(dev))
    _close16(_seq(ghip[0]), gref[0], "d conv")
    for name, a, r in zip(("W", "b", "wpe"), ghip[1:], gref[1:]):
        _close16(a, r, name)


@pytest.mark.parametrize("T", [3, 6])
def test_bf16_gpt2_block_stage_fwd_bwd(dev, T):
    """ONE GPT-2 block with LoRA + ln_f (modeling_gpt2.py:262-310, modules.py:177-186) in bf16 mode: the K-extended
    c_attn contraction, the exact-kernel LoRA-A product with bf16 backward contractions, the bf16 dqkv / d gelu-input /
    masked LayerNorm-backward operands.  Output, d input and the 8 trainable parameter gradients.  A block is itself a
    chain of 4 forward + 4 backward bf16 contractions in front of the LoRA gradients, so the absolute term is 2e-2*rms
    here (measured 1.02e-2 on lora_B at T = 6) against 1e-2 for the single-contraction stages."""
    from src.model.modules import LLMBackbone
    from tecmollm import functions as F_
    B, N = 2, 41
    cfg = R.default_config(L_in=16 * T, num_nodes=N, llm_layers=1)
    p = R.init_params(cfg, seed=45)
    g = torch.Generator().manual_seed(46)
    tok = torch.randn(B * N, T, 768, generator=g) * 0.5
    pr = {k: v.clone().requires_grad_(R.is_trainable(k)) for k, v in p.items() if k.startswith(R.P_GPT)}
    tr = tok.clone().requires_grad_(True)
    # gpt2_lora adds wpe itself; the device stage receives tokens + wpe
    ref = R.gpt2_lora(tr, pr, 1, R.BF16)
    gout = torch.randn(ref.shape, generator=g)
    names = [k for k, v in pr.items() if v.requires_grad and "wpe" not in k]
    gref = torch.autograd.grad(ref, [tr] + [pr[k] for k in names], gout)
    bb = LLMBackbone(1, include_wte=False, load_pretrained=False)
    bb.load_state_dict({k[len("llm_backbone."):]: v for k, v in p.items() if k.startswith("llm_backbone.")})
    bb = bb.to(dev).eval()
    h0 = _tm(tok + p[R.P_GPT + "wpe.weight"][:T], B, N).to(dev).requires_grad_(True)
    out = bb.forward_tm(h0, F_.DropPlan(False, 0.0, 0, BF16))
    _close16(_seq(out), ref, "block output")
    named = {"llm_backbone." + k: v for k, v in bb.named_parameters()}
    ghip = torch.autograd.grad(out, [h0] + [named[k] for k in names], _tm(gout, B, N).to(dev))
    _close16(_seq(ghip[0]), gref[0], "d tokens", 2e-2)
    for k, a, r in zip(names, ghip[1:], gref[1:]):
        _close16(a, r, k, 2e-2)


def test_bf16_head_stage_fwd_bwd(dev):
    """PredictionHead (modules.py:295-313) in bf16 mode: the 12-column output layer is exact in the forward and bf16 in
    both backward contractions."""
    from src.model.modules import PredictionHead
    from tecmollm import functions as F_
    B, N, T = 2, 45, 3
    cfg = R.default_config(L_in=48, num_nodes=N)
    p = R.init_params(cfg, seed=47)
    g = torch.Generator().manual_seed(48)
    hid = torch.randn(B * N, T, 768, generator=g)
    pr = _leaf(p, R.P_HEAD)
    hr = hid.clone().requires_grad_(True)
    ref = R.head(hr, pr, R.BF16)
    gout = torch.randn(ref.shape, generator=g)
    gref = torch.autograd.grad(ref, [hr] + list(pr.values()), gout)
    ph = PredictionHead(T * 768, 12)
    ph.load_state_dict({k[len("prediction_head."):]: v for k, v in p.items() if k.startswith(R.P_HEAD)})
    ph = ph.to(dev).eval()
    hd = _tm(hid, B, N).to(dev).requires_grad_(True)
    out = ph.forward_tm(hd, F_.DropPlan(False, 0.0, 0, BF16))             # (B, N, L_out)
    _close16(out.reshape(B * N, -1), ref, "prediction")
    named = {"prediction_head." + k: v for k, v in ph.named_parameters()}
    ghip = torch.autograd.grad(out, [hd] + [named[k] for k in pr], gout.view(B, N, -1).to(dev))
    _close16(_seq(ghip[0]), gref[0], "d hidden")
    for k, a, r in zip(pr, ghip[1:], gref[1:]):
        _close16(a, r, k)


# ----------------------------------------------------------------------------------- 2. the whole step
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("grid,thr,B", [((4, 5), 170.0, 2), ((9, 15), 150.0, 2)], ids=["N20", "N135"])
def test_bf16_full_step_against_bf16_emulating_oracle(dev, grid, thr, B, train):
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=grid[0] * grid[1])
    res = compare_forward_backward(cfg, B=B, grid=grid, threshold_km=thr, gat_graphs="per_timestep", seed=31,
                                   train=train, precision="bf16")
    # N = 20 is a 40-sequence / 120-token problem: a weight gradient there sums 120 rows and the rounding-flip noise of the
    # bf16 tensors in front of it does not average out -- it takes the SMALL40_* bars (tests/parity.py: one stated set,
    # derived there from a 20-run seed sweep); N = 135 and N = 2911 keep the standard bars, and the self-calibrated test at
    # the end of this file is the noise-independent check.
    assert_parity(res, small40=(grid == (4, 5)))
    assert res["n_grads"] == sum(R.is_trainable(k) for k in R.init_params(cfg, 0))


def test_bf16_train_mode_L96_six_tokens(dev):
    """BASELINE configs[4] shape in the bf16 mode (6 tokens, head 4608 -> 1152 -> 24), training mode."""
    cfg = R.default_config(L_in=96, L_out=24, num_nodes=20)
    # a 40-sequence problem like N20 above: the SMALL40_* bars
    assert_parity(compare_forward_backward(cfg, B=2, grid=(4, 5), threshold_km=170.0, gat_graphs="per_timestep", seed=34,
                                           train=True, precision="bf16"), small40=True)


def test_bf16_train_mode_L336_reference_default_length(dev):
    """The reference's default L_in = 336 (21 tokens) in the bf16 mode, training mode.  Its conv sequences (336 / 168 steps)
    are too long for the register-resident GroupNorm kernels -- the only ones that read / write bf16 activations -- so the
    conv blocks keep fp32 activations and take the window-GEMM routes (ops.gn_reg_ok); the arithmetic (operands rounded
    to bf16 in the loaders) is the same, and so is the oracle."""
    from tecmollm import ops
    assert not ops.gn_reg_ok(336, 20, 64) and ops.gn_reg_ok(96, 2911, 64) and ops.gn_reg_ok(24, 2911, 128)
    cfg = R.default_config(L_in=336, L_out=12, num_nodes=20, llm_layers=2)
    res = compare_forward_backward(cfg, B=2, grid=(4, 5), threshold_km=170.0, gat_graphs="per_timestep", seed=36, train=True,
                                   precision="bf16")
    # the head's first Linear contracts 21 * 768 = 16 128 bf16 products per output here, 3.5x the longest contraction of the
    # configurations the bars were calibrated on (4 608 at L_in = 96): the flip noise of its pre-activation, and with it of
    # this one weight gradient, grows like the square root of that (1.9x; measured 1.1-1.6x the standard bar)
    # (round 4, tools/diag_l336.py over three seeds: the worst tensor moves -- lora_A 1.10 at one seed, the head weight 1.39 /
    # 0.70 at the others, everything else <= 0.85 -- the rounding-flip noise of a 40-sequence problem, nothing systematic:
    # this ONE named tensor gets 2x, every other gradient the SMALL40_* bars of a 40-sequence problem)
    assert_parity(res, small40=True, elem_scale={"prediction_head.mlp.0.weight": 2.0})


def test_bf16_outlier_channels_like_a_pretrained_gpt2(dev):
    """Only config-initialised GPT-2 weights can run here (no network: modules.py:165's from_pretrained has nothing to load).
    What a pretrained trunk has and N(0, 0.02) weights do not are OUTLIER channels: a handful of residual-stream dimensions
    whose LayerNorm gains and activations are 10-50x the rest -- exactly what tensors stored as bf16 (qkv, the c_fc
    pre-activation, the gradients bf16 Linears return) would be sensitive to.  The same 40-sequence step with such a trunk
    (ln gains x30 on four channels, the matching wpe and c_fc bias entries large) must stay inside the same bars against the
    oracle that rounds where the device rounds; a store that lost the small channels next to the large ones would not."""
    from tests.parity import oracle_step, rel_err
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=20)
    p = R.init_params(cfg, seed=61)
    hot = [5, 138, 447, 600]
    with torch.no_grad():
        for k, v in p.items():
            if k.endswith(("ln_1.weight", "ln_2.weight", "ln_f.weight")):
                v[hot] *= 30.0
            elif k.endswith("wpe.weight"):
                v[:, hot] += 3.0
            elif k.endswith("mlp.c_fc.bias"):
                v[hot] += 2.0
    x, tf, y = R.synthetic_batch(2, 48, 20, cfg["spatial_in_channels_base"], 12, seed=161)
    ei, _ = R.grid_graph(4, 5, threshold_km=170.0)
    out_o, loss_o, g_o = oracle_step(cfg, p, x, tf, ei, y, None, q=device_rounding(20))
    model = build_model(cfg, p, dev, "per_timestep", precision="bf16").eval()
    tfd = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(2, 48, 20, 4)
    out = model(x.to(dev), tfd, ei.to(dev))
    loss = torch.nn.functional.huber_loss(out, y.to(dev))
    loss.backward()
    named = dict(model.named_parameters())
    res = {"fwd_rel": rel_err(out, out_o), "precision": "bf16"}
    assert res["fwd_rel"] < 2e-2, res
    errs = sorted(((rel_err(named[k].grad, g), k) for k, g in g_o.items() if g.abs().max() > 0), reverse=True)
    from tests.parity import GAT_TENSORS
    # max-norm per gradient, at twice the 40-sequence bars (measured: GATv2 stage 5.5e-2 / 4.9e-2, a conv weight 4.0e-2, the
    # rest <= 2.6e-2 -- the back-propagated signal of this trunk is dominated by four channels, so the rounding-flip noise of
    # everything in front of it doubles); a store that dropped the small channels would show as O(1)
    for e, k in errs:
        assert e < (1e-1 if k in GAT_TENSORS else 6e-2), errs[:6]


def test_bf16_full_size_batch_of_8_gradients_equal_mean_of_single_samples(dev):
    """bf16 mode as `bench.py --precision bf16` times it, eval mode, B = 8: the 66 gradients of the batch step equal the mean
    of the eight single-sample steps' gradients (tests/parity.py:batch_vs_single_sample_grads).  The forward is per-sample
    bit-exact and the batch's loss gradient is the single-sample one times 1/8 (exact, and exact through every bf16
    rounding), so the fp32 bar holds here too although the batch runs other tile heights and split-K counts."""
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=2911, c_in=10, d_emb=12)
    assert_batch_equals_mean_of_samples(batch_vs_single_sample_grads(cfg, 8, (41, 71), seed=45, precision="bf16"))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_bf16_train_mode_p0_full_size_batch_of_8_equals_eval(dev, monkeypatch):
    """Training mode at B = 8 in bf16 mode with p = 0 (every dropout site's plumbing engaged, nothing dropped) against eval
    mode on the same batch: the forward bit for bit, the 55 gradients behind the spatial stage bit for bit, the 11 of the
    spatial stage (float atomics) to 1e-5.  With the test above this ties the training-mode B = 8 step to the per-sample
    oracle checks; an oracle run of the bf16 B = 8 step (about a minute of CPU and 30 GB of host memory) is not part of the
    suite -- the fp32 one is (tests/test_gpu_model.py::test_train_mode_full_size_batch_of_8_against_oracle)."""
    import dataclasses
    import src.model.tec_mollm as TM
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=2911, c_in=10, d_emb=12)
    model = build_model(cfg, R.init_params(cfg, seed=46), dev, "per_timestep", precision="bf16")
    x, tf, y = R.synthetic_batch(8, 48, 2911, 10, 12, seed=146)
    ei = R.grid_graph()[0].to(dev)
    xd, yd = x.to(dev), y.to(dev)
    tfd = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(8, 48, 2911, 4)
    orig = TM.make_plan
    monkeypatch.setattr(TM, "make_plan", lambda m, p=0.1, precision="auto": dataclasses.replace(orig(m, p, precision), p=0.0))

    def step(train):
        model.train(train)
        model.zero_grad(set_to_none=True)
        out = model(xd, tfd, ei)
        torch.nn.functional.huber_loss(out, yd).backward()
        return out.detach().clone(), {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
    out_t, g_t = step(True)
    out_e, g_e = step(False)
    assert torch.isfinite(out_t).all() and torch.equal(out_t, out_e)
    assert len(g_t) == 66 and g_t.keys() == g_e.keys() and all(torch.isfinite(v).all() for v in g_t.values())
    spatial = [k for k in g_t if k.startswith(("spatio_temporal_embedding.", "spatial_encoder."))]
    assert len(spatial) == 11
    assert all(torch.equal(g_t[k], g_e[k]) for k in g_t if k not in spatial), \
        [k for k in g_t if k not in spatial and not torch.equal(g_t[k], g_e[k])]
    assert all(rel_err(g_t[k], g_e[k]) < 1e-5 for k in spatial), [(k, rel_err(g_t[k], g_e[k])) for k in spatial]
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_bf16_train_mode_full_size_graph_F10(dev):
    """The bf16 configuration as `bench.py --precision bf16` times it, at B = 1: training mode, dropout at every site,
    F = 10 / d_emb = 12, N = 2911, per-timestep graphs -- forward, loss and all 66 gradients against the emulating oracle."""
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=2911, c_in=10, d_emb=12)
    assert_parity(compare_forward_backward(cfg, B=1, grid=(41, 71), gat_graphs="per_timestep", seed=35, train=True,
                                           precision="bf16"))


# ----------------------------------------------------------------------------------- 3. self-calibrated
def test_bf16_device_is_as_close_to_the_oracle_as_the_oracle_is_to_itself(dev):
    """The distance device <-> emulating oracle, per gradient tensor, against the oracle's own sensitivity: the same
    oracle with x and every parameter perturbed by a relative 1e-6 (what separates the two implementations in fp32 mode:
    summation order).  Both distances sit at the bf16 noise floor; the device must not be farther than 2x the oracle's own
    wobble (+ a 2e-3 floor for tensors whose self-distance happens to be small), and on average not farther than 1.3x.
    The FP32 oracle and the forward-only emulation are measurably farther away than the full emulation."""
    grid, B = (9, 15), 2
    N = grid[0] * grid[1]
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=N)
    p = R.init_params(cfg, seed=51)
    x, tf, y = R.synthetic_batch(B, 48, N, 6, 12, seed=151)
    ei, _ = R.grid_graph(grid[0], grid[1])
    model = build_model(cfg, p, dev, "per_timestep", precision="bf16").eval()
    tfd = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(B, 48, N, 4)
    out = model(x.to(dev), tfd, ei.to(dev))
    torch.nn.functional.huber_loss(out, y.to(dev)).backward()
    named = dict(model.named_parameters())
    out_o, _, g_o = oracle_step(cfg, p, x, tf, ei, y, None, q=device_rounding(N))
    gen = torch.Generator().manual_seed(52)

    def wobble(t):
        return t * (1.0 + 1e-6 * torch.randn(t.shape, generator=gen)) if t.is_floating_point() else t
    p2 = {k: wobble(v) for k, v in p.items()}
    out_s, _, g_s = oracle_step(cfg, p2, wobble(x), tf, ei, y, None, q=device_rounding(N))
    _, _, g_32 = oracle_step(cfg, p, x, tf, ei, y, None, q=R.FP32)
    _, _, g_fo = oracle_step(cfg, p, x, tf, ei, y, None, q=R.BF16_FORWARD_ONLY)
    keys = [k for k, g in g_o.items() if g.abs().max() > 0]
    d_dev = np.array([l2_rel(named[k].grad, g_o[k]) for k in keys])
    d_self = np.array([l2_rel(g_s[k], g_o[k]) for k in keys])
    d_32 = np.array([l2_rel(named[k].grad, g_32[k]) for k in keys])
    d_fo = np.array([l2_rel(named[k].grad, g_fo[k]) for k in keys])
    worst = int(np.argmax(d_dev / (d_self + 1e-3)))
    assert (d_dev <= 2.0 * d_self + 2e-3).all(), (keys[worst], d_dev[worst], d_self[worst])
    assert d_dev.mean() <= 1.3 * d_self.mean(), (d_dev.mean(), d_self.mean())
    assert l2_rel(out, out_o) <= 2.0 * l2_rel(out_s, out_o) + 2e-3
    # ... and the emulation is the better model of what the device computes
    assert d_dev.mean() < d_fo.mean() < d_32.mean(), (d_dev.mean(), d_fo.mean(), d_32.mean())


@pytest.mark.parametrize("var", ["TECM_FUSE_HEAD", "TECM_BF16_TN", "TECM_CONV_STATS", "TECM_GN_BWD_SPLIT", "TECM_BF16_DMA"])
def test_bf16_diagnostic_switches_keep_the_older_kernels_working(dev, var, monkeypatch):
    """INTEGRATION.md lists environment switches that route a stage back to the kernel it had before round 4 (A/B
    diagnostics): each of those routes still gives the same step (the 40-sequence bars, parity.SMALL40_*)."""
    monkeypatch.setenv(var, "0")
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=20)
    res = compare_forward_backward(cfg, B=2, grid=(4, 5), threshold_km=170.0, gat_graphs="per_timestep", seed=31, train=True,
                                   precision="bf16")
    assert_parity(res, small40=True)
