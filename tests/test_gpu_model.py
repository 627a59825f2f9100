"""GPU parity tests of the stages and of the whole TEC_MoLLM step against the CPU oracle and against the
golden vectors generated from the reference's own classes (tests/golden/, oracle/make_golden.py).
Tolerance: 1e-3 relative (north star: "within 1e-3 rel fp32"); embedding gather bit-exact."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests.parity import (assert_batch_equals_mean_of_samples, assert_close, assert_parity, batch_vs_single_sample_grads,
                          build_model, compare_forward_backward, device_rounding, elem_err, oracle_step, rel_err)

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _spatial_inputs(cfg, B, L, grid, seed, thr=170.0):
    N = grid[0] * grid[1]
    p = R.init_params(cfg, seed=seed)
    x, tf, _ = R.synthetic_batch(B, L, N, cfg["spatial_in_channels_base"], 12, seed=seed + 1)
    ei, _ = R.grid_graph(grid[0], grid[1], threshold_km=thr)
    return p, x, tf, ei


def _run_spatial(p, x, tf, ei, dev, R_graphs, plan=None, tf_dev=None):
    from tecmollm import functions as F_
    from tecmollm import graph
    B, L, N, _ = x.shape
    meta = graph.get(ei.to(dev), N, dev, p[R.P_EMB + "node_embedding.weight"].shape[1])
    names = [R.P_EMB + f"{n}_embedding.weight" for n in ("node", "tod", "doy", "year", "season")] + \
            [R.P_GAT + n for n in ("lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "att", "bias")]
    ps = [p[n].to(dev).requires_grad_(True) for n in names]
    if tf_dev is None:
        tf_dev = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(B, L, N, 4)
    plan = plan or F_.DropPlan(False, 0.0, 0)
    out = F_.SpatialFn.apply(x.to(dev), tf_dev, *ps, meta, 2, R_graphs, plan)
    return out, ps, names


@pytest.mark.parametrize("mode", ["reference", "per_timestep"])
@pytest.mark.parametrize("grid,thr", [((3, 4), 170.0), ((9, 15), 150.0)])
def test_spatial_fwd_bwd_matches_oracle(dev, mode, grid, thr):
    cfg = R.default_config(num_nodes=grid[0] * grid[1])
    p, x, tf, ei = _spatial_inputs(cfg, 2, 5, grid, seed=3, thr=thr)
    B, L, N = 2, 5, grid[0] * grid[1]
    gwe = 1 if mode == "reference" else None
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items() if k.startswith((R.P_EMB, R.P_GAT))}
    ref = R.spatial(R.embed(x, tf, pr), ei, pr, 2, gwe)                        # (L*B, N, C)
    ref_tm = ref.view(L, B, N, 22).permute(1, 0, 2, 3)
    out, ps, names = _run_spatial(p, x, tf, ei, dev, 1 if mode == "reference" else B * L)
    assert out.shape == (B, L, N, 24)
    assert_close(out[..., :22], ref_tm)
    assert float(out[..., 22:].abs().max()) == 0.0
    gout = torch.randn(B, L, N, 22, generator=torch.Generator().manual_seed(9))
    gref = torch.autograd.grad(ref_tm, [pr[n] for n in names], gout)
    gpad = torch.zeros(B, L, N, 24)
    gpad[..., :22] = gout
    ghip = torch.autograd.grad(out, ps, gpad.to(dev))
    for n, a, b in zip(names, ghip, gref):
        assert_close(a, b, n)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("mode", ["reference", "per_timestep"])
@pytest.mark.parametrize("grid,thr,cin", [((3, 4), 170.0, 6), ((9, 15), 150.0, 6), ((12, 30), 150.0, 10)])
def test_spatial_forward_second_formulation_matches_the_first(dev, grid, thr, cin, mode, train, monkeypatch):
    """csrc/spatial_fwd2.hip (round 5: one (tile, graph) item per block, transforms split into node part + per-graph vector
    + Cin-wide per-row part) against csrc/spatial_fwd.hip on the same call: same tiles, same mask indices, another
    summation order in the transforms -- fp32 rounding apart.  Both graph modes, both feature widths (F = 6 / d_emb = 16,
    F = 10 / d_emb = 12), several tiles (N = 360), dropout of the attention coefficients on and off; and the selection:
    per-node time features stay on the first kernel."""
    from tecmollm import functions as F_
    from tecmollm import ops
    N = grid[0] * grid[1]
    cfg = R.default_config(num_nodes=N, c_in=cin, d_emb=22 - cin)
    p, x, tf, ei = _spatial_inputs(cfg, 2, 5, grid, seed=13, thr=thr)
    plan = F_.DropPlan(True, 0.1, 4711) if train else None
    R_graphs = 1 if mode == "reference" else 10
    rec = []
    real = F_.lib

    class Spy:                                              # which entry point served the call
        def __getattr__(self, name):
            fn = getattr(real(), name)
            if name in ("tecm_spatial_fwd", "tecm_spatial_fwd2"):
                rec.append(name)
            return fn
    monkeypatch.setattr(F_, "lib", lambda: Spy())
    out2, _, _ = _run_spatial(p, x, tf, ei, dev, R_graphs, plan=plan)
    monkeypatch.setenv("TECM_SPATIAL_V2", "0")
    out1, _, _ = _run_spatial(p, x, tf, ei, dev, R_graphs, plan=plan)
    assert rec == ["tecm_spatial_fwd2", "tecm_spatial_fwd"], rec
    assert torch.isfinite(out2).all() and float(out2[..., 22:].abs().max()) == 0.0
    assert float((out2 - out1).abs().max()) < 2e-6 * float(out1.abs().max())
    if train:
        ev, _, _ = _run_spatial(p, x, tf, ei, dev, R_graphs)
        assert float((out2 - ev).abs().max()) > 1e-3          # the mask really is applied
    # per-node time features: not served by the second formulation
    monkeypatch.delenv("TECM_SPATIAL_V2")
    rec.clear()
    g = torch.Generator().manual_seed(6)
    tfn = torch.stack([torch.randint(0, hi, (2, 5, N), generator=g) for hi in (12, 366, 13, 4)], -1).float()
    _run_spatial(p, x, tfn, ei, dev, R_graphs, tf_dev=tfn.to(dev))
    assert rec == ["tecm_spatial_fwd"], rec


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("mode", ["reference", "per_timestep"])
@pytest.mark.parametrize("grid,thr,cin", [((3, 4), 170.0, 6), ((12, 30), 150.0, 10)])
def test_spatial_backward_second_formulation_matches_the_first(dev, grid, thr, cin, mode, train, monkeypatch):
    """csrc/spatial_bwd2.hip against csrc/spatial_bwd.hip on the same call: all eleven parameter gradients (five embedding
    tables, lin_l / lin_r weight and bias, att, bias) agree to fp32 summation order -- both graph modes, both feature widths,
    several tiles and graph chunks (N = 360, 10 graphs), dropout of the attention coefficients on and off."""
    from tecmollm import functions as F_
    N = grid[0] * grid[1]
    cfg = R.default_config(num_nodes=N, c_in=cin, d_emb=22 - cin)
    p, x, tf, ei = _spatial_inputs(cfg, 2, 5, grid, seed=17, thr=thr)
    plan = F_.DropPlan(True, 0.1, 4711) if train else None
    R_graphs = 1 if mode == "reference" else 10
    gout = torch.randn(2, 5, N, 24, generator=torch.Generator().manual_seed(3)).to(dev)
    gout[..., 22:] = 0
    rec = []
    real = F_.lib

    class Spy:
        def __getattr__(self, name):
            if name in ("tecm_spatial_bwd", "tecm_spatial_bwd2"):
                rec.append(name)
            return getattr(real(), name)
    monkeypatch.setattr(F_, "lib", lambda: Spy())
    out, ps, names = _run_spatial(p, x, tf, ei, dev, R_graphs, plan=plan)
    g2 = torch.autograd.grad(out, ps, gout)
    monkeypatch.setenv("TECM_SPATIAL_BWD2", "0")
    out, ps, names = _run_spatial(p, x, tf, ei, dev, R_graphs, plan=plan)
    g1 = torch.autograd.grad(out, ps, gout)
    assert rec == ["tecm_spatial_bwd2", "tecm_spatial_bwd"], rec
    for n, a, b in zip(names, g2, g1):
        assert torch.isfinite(a).all(), n
        assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()) + 1e-7, (n, float((a - b).abs().max()), float(b.abs().max()))


def test_spatial_general_time_features_per_node(dev):
    """time_features that really vary over N (not a stride-0 view) take the per-node path."""
    grid = (4, 5)
    cfg = R.default_config(num_nodes=20)
    p, x, _, ei = _spatial_inputs(cfg, 2, 3, grid, seed=5)
    g = torch.Generator().manual_seed(6)
    tf = torch.stack([torch.randint(0, hi, (2, 3, 20), generator=g) for hi in (12, 366, 13, 4)], -1).float()
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items() if k.startswith((R.P_EMB, R.P_GAT))}
    ref = R.spatial(R.embed(x, tf, pr), ei, pr, 2, None).view(3, 2, 20, 22).permute(1, 0, 2, 3)
    out, ps, names = _run_spatial(p, x, tf, ei, dev, 6, tf_dev=tf.to(dev))
    assert_close(out[..., :22], ref)
    gout = torch.randn(2, 3, 20, 22, generator=g)
    gref = torch.autograd.grad(ref, [pr[n] for n in names], gout)
    gpad = torch.zeros(2, 3, 20, 24)
    gpad[..., :22] = gout
    ghip = torch.autograd.grad(out, ps, gpad.to(dev))
    for n, a, b in zip(names, ghip, gref):
        assert_close(a, b, n)


def test_embedding_gather_bit_exact_against_reference_golden(dev, golden_dir):
    """With lin_l = 0 and bias = 0 the fused kernel returns h = cat([x, emb]) unchanged, so the embedding
    gather + sums can be compared BIT-EXACTLY with the reference's SpatioTemporalEmbedding at N = 2911."""
    g = np.load(os.path.join(golden_dir, "embed_fullN.npz"))
    cfg = R.default_config(num_nodes=2911)
    p = R.init_params(cfg, seed=int(g["seed"]))
    for n in ("lin_l.weight", "lin_l.bias", "bias"):
        p[R.P_GAT + n] = torch.zeros_like(p[R.P_GAT + n])
    x, _, _ = R.synthetic_batch(1, 2, 2911, 6, 12, seed=int(g["data_seed"]))
    tf = torch.from_numpy(g["tf"]).unsqueeze(-2).expand(-1, -1, 2911, -1)
    ei, _ = R.grid_graph()
    for Rg in (1, 2):
        out, _, _ = _run_spatial(p, x, tf, ei, dev, Rg)
        assert torch.equal(out[..., 6:22].cpu(), torch.from_numpy(g["out_emb"]))
        assert torch.equal(out[..., :6].cpu(), x)


@pytest.mark.parametrize("tag", ["L48", "L96"])
def test_temporal_encoder_matches_reference_golden(dev, golden_dir, tag):
    from src.model.modules import TemporalEncoder
    g = np.load(os.path.join(golden_dir, f"temporal_{tag}.npz"))
    cfg = R.default_config(L_in=int(g["L_in"]), num_nodes=8)
    p = R.init_params(cfg, seed=int(g["seed"]))
    te = TemporalEncoder(22, cfg["temporal_channel_list"], cfg["temporal_strides"], cfg["patch_len"], 768)
    te.load_state_dict({k[len("temporal_encoder."):]: v for k, v in p.items() if k.startswith("temporal_encoder.")})
    te = te.to(dev)
    x = torch.from_numpy(g["x"]).to(dev)
    out = te(x)
    assert_close(out, torch.from_numpy(g["out"]))
    blk0 = te.conv_embedder.embedder[0](x.permute(0, 2, 1).contiguous())
    assert_close(blk0, torch.from_numpy(g["block0"]))


def test_prediction_head_matches_reference_golden(dev, golden_dir):
    from src.model.modules import PredictionHead
    g = np.load(os.path.join(golden_dir, "head.npz"))
    cfg = R.default_config(num_nodes=8)
    p = R.init_params(cfg, seed=int(g["seed"]))
    ph = PredictionHead(2304, 12).eval()
    ph.load_state_dict({k[len("prediction_head."):]: v for k, v in p.items() if k.startswith("prediction_head.")})
    out = ph.to(dev)(torch.from_numpy(g["x"]).to(dev))
    assert_close(out, torch.from_numpy(g["out"]))


@pytest.mark.parametrize("tag", ["T3", "T6"])
def test_gpt2_trunk_matches_transformers_golden(dev, golden_dir, tag):
    from src.model.modules import LLMBackbone
    g = np.load(os.path.join(golden_dir, f"gpt2_{tag}.npz"))
    T = int(g["T"])
    cfg = R.default_config(L_in=16 * T, num_nodes=8)
    p = R.init_params(cfg, seed=int(g["seed"]))
    bb = LLMBackbone(3, include_wte=False, load_pretrained=False).eval()
    sd = {k[len("llm_backbone."):]: v for k, v in p.items() if k.startswith("llm_backbone.")}
    for i in range(3):
        sd[f"model.base_model.model.h.{i}.attn.c_attn.lora_B.default.weight"] = torch.zeros(2304, 32)
    bb.load_state_dict(sd)
    out = bb.to(dev)(torch.from_numpy(g["x"]).to(dev), None)
    assert_close(out, torch.from_numpy(g["out"]))


@pytest.mark.parametrize("mode", ["reference", "per_timestep"])
def test_full_step_small(dev, mode):
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=12)
    res = compare_forward_backward(cfg, B=2, grid=(3, 4), threshold_km=170.0, gat_graphs=mode, seed=3)
    assert_parity(res)
    assert res["n_grads"] == sum(R.is_trainable(k) for k in R.init_params(cfg, 0))


def test_full_step_L48_medium_graph(dev):
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=9 * 15)
    assert_parity(compare_forward_backward(cfg, B=3, grid=(9, 15), gat_graphs="per_timestep", seed=5))


def test_full_step_L96_stress_shape(dev):
    cfg = R.default_config(L_in=96, L_out=24, num_nodes=20)
    assert_parity(compare_forward_backward(cfg, B=2, grid=(4, 5), threshold_km=170.0, gat_graphs="per_timestep", seed=6,
                                           use_fused_huber=False))


def test_full_step_L336_six_layers_T21(dev):
    """The reference's 4-GPU script shape (scripts/train_with_dynamic_naming.sh:4-11): L_in=336, 6 GPT-2 layers
    -> 21 tokens per sequence, head 16128 -> 4032 -> 12."""
    cfg = R.default_config(L_in=336, L_out=12, num_nodes=6, llm_layers=6)
    assert_parity(compare_forward_backward(cfg, B=1, grid=(2, 3), threshold_km=170.0, gat_graphs="per_timestep", seed=8))


def test_full_step_L192_T12(dev):
    """L_in=192 -> 12 tokens per sequence (the other compile-time attention specialisation beyond T <= 6)."""
    cfg = R.default_config(L_in=192, L_out=12, num_nodes=6, llm_layers=2)
    assert_parity(compare_forward_backward(cfg, B=2, grid=(2, 3), threshold_km=170.0, gat_graphs="per_timestep", seed=9))


def test_full_size_graph_B1_against_oracle(dev):
    """BASELINE config shape (L_in=48, N=2911, E=20924) at B=1: forward + every trainable gradient."""
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=2911)
    assert_parity(compare_forward_backward(cfg, B=1, grid=(41, 71), gat_graphs="per_timestep", seed=7), kink=True)


def test_full_size_graph_F10_demb12_the_timed_workload(dev):
    """The workload bench.py times: raw feature width F = 10 with d_emb = 12 (still C = 22), N = 2911,
    per-timestep graphs -- forward, loss and every trainable gradient against the oracle, eval mode."""
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=2911, c_in=10, d_emb=12)
    assert_parity(compare_forward_backward(cfg, B=1, grid=(41, 71), gat_graphs="per_timestep", seed=13), kink=True)


def test_full_size_graph_L96_L24_stress_config(dev):
    """BASELINE configs[4] per-GPU shape at full graph size: L_in=96 / L_out=24 (6 tokens, head 4608 -> 1152 -> 24),
    N = 2911, F = 10."""
    cfg = R.default_config(L_in=96, L_out=24, num_nodes=2911, c_in=10, d_emb=12)
    assert_parity(compare_forward_backward(cfg, B=1, grid=(41, 71), gat_graphs="per_timestep", seed=14), kink=True)


# ----------------------------------------------------------------------------- training mode (every dropout site on)
@pytest.mark.parametrize("mode", ["reference", "per_timestep"])
def test_train_mode_full_step_small_with_mirrored_masks(dev, mode):
    """Training-mode forward + all gradients against the oracle fed with the NumPy mirror of the device masks at every
    dropout site of the reference: GAT alpha (modules.py:333), LoRA input (:181), GPT-2 embd/attn/resid, post-LLM
    (tec_mollm.py:115), head (modules.py:289)."""
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=12)
    res = compare_forward_backward(cfg, B=2, grid=(3, 4), threshold_km=170.0, gat_graphs=mode, seed=21, train=True)
    assert_parity(res)
    # the masks really bite: the same step in eval mode is far away
    ev = compare_forward_backward(cfg, B=2, grid=(3, 4), threshold_km=170.0, gat_graphs=mode, seed=21, train=False)
    assert_parity(ev)


def test_train_mode_L48_medium_graph_F10(dev):
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=9 * 15, c_in=10, d_emb=12)
    assert_parity(compare_forward_backward(cfg, B=3, grid=(9, 15), gat_graphs="per_timestep", seed=22, train=True))


def test_train_mode_L96_six_tokens(dev):
    cfg = R.default_config(L_in=96, L_out=24, num_nodes=20)
    assert_parity(compare_forward_backward(cfg, B=2, grid=(4, 5), threshold_km=170.0, gat_graphs="per_timestep", seed=23,
                                           train=True))


def test_train_mode_full_size_graph_F10_the_timed_configuration(dev):
    """Exactly what BENCH times, at B = 1: training mode, dropout p = 0.1 at every site, F = 10 / d_emb = 12,
    N = 2911, per-timestep graphs; forward, loss and all 66 trainable gradients within 1e-3 of the oracle."""
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=2911, c_in=10, d_emb=12)
    assert_parity(compare_forward_backward(cfg, B=1, grid=(41, 71), gat_graphs="per_timestep", seed=24, train=True), kink=True)


# ----------------------------------------------------------------------------- B = 8: the batch bench.py times
# Several choices are keyed by the batch: spatial_bwd2's graph-chunk count (capped at G = B*L graphs: 48 at B = 1, 384 at
# B = 8), the bf16 GEMMs' tile height (M = 8 733 vs 69 864 token rows) and every weight-gradient GEMM's split-K count
# (pick_split_k, from K = rows).  The B = 1 tests above never reach the B = 8 choices.
@pytest.mark.parametrize("L_in,L_out", [(48, 12), (96, 24)], ids=["timed", "L96_L24"])
def test_full_size_batch_of_8_gradients_equal_mean_of_single_samples(dev, L_in, L_out):
    """Eval mode, N = 2911, F = 10 / d_emb = 12, per-timestep graphs: the 66 gradients of one B = 8 step equal the mean of
    the eight B = 1 steps' gradients (each of which the oracle tests above verify) to fp32 summation order
    (tests/parity.py:batch_vs_single_sample_grads).  L_in = 96 / L_out = 24 is BASELINE configs[4]."""
    cfg = R.default_config(L_in=L_in, L_out=L_out, num_nodes=2911, c_in=10, d_emb=12)
    assert_batch_equals_mean_of_samples(batch_vs_single_sample_grads(cfg, 8, (41, 71), seed=41 + L_in))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_train_mode_full_size_batch_of_8_against_oracle(dev):
    """The timed step itself: training mode (dropout p = 0.1 at every site; the masks are keyed by the global row, which
    includes b, so the per-sample comparison above cannot cover it), B = 8, N = 2911, F = 10 / d_emb = 12 -- forward, loss
    and all 66 gradients against the oracle fed the mirrored masks.
    The standard bars for the forward, the loss and the 57 gradients outside KINK_TENSORS.  The nine tensors whose gradient
    passes through GATv2's LeakyReLU kink (tests/parity.py) do not meet the B = 1 kink bar at 384 graphs, and neither does
    the ORACLE against itself: with inputs and parameters perturbed by a relative 1e-6 it moves the node-table gradient by
    2.9e-3 max-norm / 2.07x the kink bar (seed 25; seed 26: 2.1e-3 / 1.74x).  The device here: 3.4e-3 / 2.53x, on two
    neighbouring rows (1015, 1016) that both spatial backward formulations (spatial_bwd2 and spatial_bwd) give identically;
    lin_r.weight 1.1e-3 / 1.25x.  These nine tensors get 1e-2 max-norm and 4x the kink bar; a wrong mask, chunk or slab in
    the spatial backward is O(1e-2..1) there and breaks the standard bars of att / bias anyway."""
    from tests.parity import KINK_TENSORS
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=2911, c_in=10, d_emb=12)
    res = compare_forward_backward(cfg, B=8, grid=(41, 71), gat_graphs="per_timestep", seed=25, train=True)
    brief = {k: v for k, v in res.items() if k != "per_param"}
    assert res["n_grads"] == 66 and res["frozen_with_grad"] == [], brief
    assert res["fwd_rel"] < TOL and res["loss_rel"] < TOL and res["fwd_elem"] < 1.0, brief
    assert res["grad_elem_max"] < 1.0, brief                          # every tensor outside KINK_TENSORS, element-wise
    for k, (e, _, _) in res["per_param"].items():
        assert e < (1e-2 if k in KINK_TENSORS else TOL), (k, e, brief)
    assert res["kink_elem_max"] < 4.0, brief
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_gat_alpha_dropout_matches_oracle_alpha_mult(dev):
    """The attention-coefficient dropout of GATv2Conv (modules.py:333) on its own: spatial stage forward and every
    gradient with the mirrored alpha mask, on an irregular multigraph (duplicate edges, explicit self loops, a hub)."""
    from tests.parity import device_masks
    from tecmollm import functions as F_
    N, B, L = 150, 2, 3
    cfg = R.default_config(num_nodes=N)
    cfg["temporal_seq_len"] = 16 * 3                      # only used for the shapes of the masks we do not need here
    p = R.init_params(cfg, seed=8)
    x, tf, _ = R.synthetic_batch(B, L, N, cfg["spatial_in_channels_base"], 12, seed=9)
    g = torch.Generator().manual_seed(10)
    src = torch.randint(0, N, (400,), generator=g)
    dst = torch.randint(0, N, (400,), generator=g)
    hub = torch.stack([torch.arange(40, 100), torch.full((60,), 3)])
    loops = torch.stack([torch.arange(0, 20), torch.arange(0, 20)])
    dup = torch.stack([src[:50], dst[:50]])
    ei = torch.cat([torch.stack([src, dst]), hub, loops, dup], 1)
    base_seed = 987654321
    mcfg = dict(cfg, temporal_seq_len=L, temporal_strides=[1, 1], patch_len=1, llm_layers=0)
    masks = device_masks(mcfg, B, ei, base_seed, "per_timestep")
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items() if k.startswith((R.P_EMB, R.P_GAT))}
    ref = R.spatial(R.embed(x, tf, pr), ei, pr, 2, None, alpha_mult=masks["gat"])
    ref_tm = ref.view(L, B, N, 22).permute(1, 0, 2, 3)
    plan = F_.DropPlan(True, 0.1, base_seed)
    out, ps, names = _run_spatial(p, x, tf, ei, dev, B * L, plan=plan)
    assert rel_err(out[..., :22], ref_tm) < TOL and elem_err(out[..., :22], ref_tm) < 1.0
    noplan, _, _ = _run_spatial(p, x, tf, ei, dev, B * L)
    assert rel_err(noplan[..., :22], ref_tm) > 1e-2                      # the mask matters
    gout = torch.randn(B, L, N, 22, generator=torch.Generator().manual_seed(11))
    gref = torch.autograd.grad(ref_tm, [pr[n] for n in names], gout)
    gpad = torch.zeros(B, L, N, 24)
    gpad[..., :22] = gout
    ghip = torch.autograd.grad(out, ps, gpad.to(dev))
    for n, a, b in zip(names, ghip, gref):
        assert_close(a, b, n)


def test_three_arg_call_and_output_contract(dev):
    """test.py:37 calls model(x, tf, edge_index) with three arguments; output is (B, L_out, N, 1)."""
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=12)
    p = R.init_params(cfg, seed=1)
    model = build_model(cfg, p, dev).eval()
    x, tf, _ = R.synthetic_batch(2, 16, 12, 6, 12, seed=2)
    ei, _ = R.grid_graph(3, 4, threshold_km=170.0)
    with torch.no_grad():
        out = model(x.to(dev), tf.to(dev), ei.to(dev))
        out2 = model(x.to(dev), tf.to(dev), ei.to(dev), None)
    assert out.shape == (2, 12, 12, 1) and torch.equal(out, out2)
    model.llm_backbone.model.gradient_checkpointing_enable()        # train.py:70-73 must not raise
    with pytest.raises(Exception):
        model(x, tf, ei)                                            # CPU tensors: no silent fallback


def test_training_mode_dropout_is_active_and_reproducible(dev):
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=12)
    p = R.init_params(cfg, seed=1)
    model = build_model(cfg, p, dev, "per_timestep").train()
    x, tf, y = R.synthetic_batch(2, 16, 12, 6, 12, seed=2)
    ei, _ = R.grid_graph(3, 4, threshold_km=170.0)
    xd, tfd, eid = x.to(dev), tf.to(dev), ei.to(dev)
    out_a = model(xd, tfd, eid)
    out_b = model(xd, tfd, eid)
    assert not torch.equal(out_a, out_b)                            # fresh masks every call
    model.eval()
    with torch.no_grad():
        e = model(xd, tfd, eid)
    assert float((out_a - e).abs().max()) > 1e-4
    # backward with dropout on runs and yields finite gradients for every trainable parameter
    model.train()
    loss = torch.nn.functional.huber_loss(model(xd, tfd, eid), y.to(dev))
    loss.backward()
    for n, q in model.named_parameters():
        if q.requires_grad:
            assert q.grad is not None and torch.isfinite(q.grad).all(), n


def test_train_mode_p0_equals_eval(dev):
    """With p = 0 the training-mode path (all dropout plumbing engaged) must equal eval exactly."""
    from src.model import modules as M
    from tecmollm import functions as F_
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=12)
    p = R.init_params(cfg, seed=1)
    model = build_model(cfg, p, dev).train()
    x, tf, _ = R.synthetic_batch(2, 16, 12, 6, 12, seed=2)
    ei, _ = R.grid_graph(3, 4, threshold_km=170.0)
    orig = M.make_plan
    try:
        import src.model.tec_mollm as TM
        TM.make_plan = lambda m, p=0.1, precision="auto": F_.DropPlan(True, 0.0, 1)
        a = model(x.to(dev), tf.to(dev), ei.to(dev))
    finally:
        TM.make_plan = orig
    model.eval()
    b = model(x.to(dev), tf.to(dev), ei.to(dev))
    assert torch.equal(a, b)


# ----------------------------------------------------------------------------- bf16 MFMA mode (BASELINE configs[2])
def _bf16_inputs(cfg, B, grid, seed, thr=170.0):
    N = grid[0] * grid[1]
    p = R.init_params(cfg, seed=seed)
    x, tf, y = R.synthetic_batch(B, cfg["temporal_seq_len"], N, 6, cfg["prediction_horizon"], seed=seed + 100)
    ei, _ = R.grid_graph(grid[0], grid[1], threshold_km=thr)
    return p, x, tf, y, ei


def test_bf16_forward_matches_bf16_emulating_oracle(dev):
    """Operands of every GEMM the bf16 kernel serves are rounded to bf16 in the oracle too (ref_cpu.forward(q=R.BF16)).
    What is left is summation order PLUS rounding flips amplified along the chain (tests/parity.py: RTOL_BF16_MODEL):
    max-norm observed 4.7e-3.  Backward and the per-stage bars: tests/test_gpu_bf16_model.py.  The GEMM itself is checked at 2e-4 against rounded
    operands in tests/test_gpu_bf16.py."""
    from tests.parity import ATOL_RMS_BF16_MODEL, RTOL_BF16_MODEL
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=20)
    p, x, tf, y, ei = _bf16_inputs(cfg, 2, (4, 5), seed=11)
    ref = R.forward(x, tf, ei, p, cfg, None, q=device_rounding(cfg["num_nodes"]))
    model = build_model(dict(cfg, precision="bf16"), p, dev, "per_timestep").eval()
    with torch.no_grad():
        out = model(x.to(dev), tf.to(dev), ei.to(dev))
        model.precision = "fp32"
        out32 = model(x.to(dev), tf.to(dev), ei.to(dev))
    assert_close(out, ref, "bf16 forward", RTOL_BF16_MODEL, ATOL_RMS_BF16_MODEL)
    assert rel_err(out32, ref) > rel_err(out, ref)     # fp32 mode is farther from the bf16 emulation than bf16 mode


def test_bf16_autocast_selects_bf16_and_full_step_tracks_fp32_oracle(dev):
    """Under torch.autocast(bf16) (how train.py:68 calls the model) precision 'auto' picks the bf16 kernels.
    Forward/backward vs the FP32 oracle within bf16 noise (operands carry 8 significant bits): a sanity bound only --
    the parity statement of the bf16 mode is the emulating-oracle tests below."""
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=12)
    p, x, tf, y, ei = _bf16_inputs(cfg, 2, (3, 4), seed=12)
    out_ref, loss_ref, grads_ref = oracle_step(cfg, p, x, tf, ei, y, None)
    model = build_model(cfg, p, dev, "per_timestep").eval()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(x.to(dev), tf.to(dev), ei.to(dev))
        loss = torch.nn.functional.huber_loss(out.float(), y.to(dev))
    with torch.no_grad():
        out32 = model(x.to(dev), tf.to(dev), ei.to(dev))
    assert out.dtype == torch.float32
    assert 1e-5 < rel_err(out, out32) < 3e-2
    assert rel_err(out, out_ref) < 3e-2
    loss.backward()
    named = dict(model.named_parameters())
    worst = max(rel_err(named[k].grad, g) for k, g in grads_ref.items() if g.abs().max() > 0)
    assert worst < 8e-2, worst
    # the same gradients against the oracle that rounds what the device rounds: within the model-level bf16 bar
    # (tests/parity.py RTOL_BF16_MODEL; in this 24-sequence problem the rounding-flip noise alone is 0.9-1.4e-2 whichever
    # tensors are stored as bf16 -- tools/diag_y16.py over three seeds, round 4 -- so the fp32 oracle is no further away
    # here; what the emulating oracle removes is bias, and the stage-level tests of test_gpu_bf16_model.py measure that)
    from tests.parity import RTOL_BF16_MODEL
    _, _, grads_16 = oracle_step(cfg, p, x, tf, ei, y, None, q=device_rounding(cfg["num_nodes"]))
    worst16 = max(rel_err(named[k].grad, g) for k, g in grads_16.items() if g.abs().max() > 0)
    assert worst16 < RTOL_BF16_MODEL and worst16 < worst + 5e-3, (worst16, worst)   # ... and no farther than the fp32 oracle (+ noise)


def test_second_forward_before_backward_of_the_same_layer_is_refused(dev):
    """The K-extended c_attn operand [W ; 2 B^T] the backward reads lives in a per-parameter cache buffer that the next
    forward of the same layer rewrites through a raw pointer (torch's version counter cannot see it).  A backward whose
    operand was overwritten meanwhile must raise, not differentiate against the wrong lora_B."""
    from tecmollm import TecmError
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=6, llm_layers=1)
    p = R.init_params(cfg, seed=23)
    x, tf, y = R.synthetic_batch(1, 16, 6, cfg["spatial_in_channels_base"], 12, seed=5)
    ei, _ = R.grid_graph(2, 3, threshold_km=2000.0)
    model = build_model(cfg, p, dev, "per_timestep").eval()
    out1 = model(x.to(dev), tf.to(dev), ei.to(dev))
    out2 = model(x.to(dev), tf.to(dev), ei.to(dev))              # same layer, same cache buffer: generation moves on
    out2.sum().backward()                                         # the latest forward's backward is fine
    with pytest.raises(TecmError, match="rewritten by a later forward"):
        out1.sum().backward()


def test_frozen_weight_transposes_follow_the_parameter(dev):
    """The forward GEMMs read cached [N][K] copies of the frozen GPT-2 weights: a second model (whose parameters may
    reuse the ids / addresses of a collected one) and an in-place weight reload must both be picked up."""
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=6, llm_layers=1)
    outs = []
    for seed in (21, 22):
        p = R.init_params(cfg, seed=seed)
        x, tf, y = R.synthetic_batch(1, 16, 6, cfg["spatial_in_channels_base"], 12, seed=5)
        ei, _ = R.grid_graph(2, 3, threshold_km=2000.0)
        model = build_model(cfg, p, dev, "per_timestep").eval()
        tfd = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(1, 16, 6, 4)
        with torch.no_grad():
            out = model(x.to(dev), tfd, ei.to(dev))
        ref = R.forward(x, tf, ei, p, cfg, None)
        assert rel_err(out, ref) < 1e-3
        outs.append(out)
        del model
    # same module object, weights replaced in place (load_state_dict): the cache must refresh
    p1, p2 = R.init_params(cfg, seed=31), R.init_params(cfg, seed=32)
    model = build_model(cfg, p1, dev, "per_timestep").eval()
    with torch.no_grad():
        a = model(x.to(dev), tfd, ei.to(dev))
        model.load_state_dict(p2, strict=True)
        b = model(x.to(dev), tfd, ei.to(dev))
    assert rel_err(a, R.forward(x, tf, ei, p1, cfg, None)) < 1e-3
    assert rel_err(b, R.forward(x, tf, ei, p2, cfg, None)) < 1e-3


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_full_size_batch_of_8_properties(dev, precision):
    """BASELINE configs[1] / configs[2] size (B=8, L_in=48, N=2911, F=10; fp32 and bf16 mode) through properties that need
    no oracle run:
    samples are independent (row b of the batch == the same sample run alone, bit for bit: no kernel mixes rows of
    different samples and none of the forward kernels uses atomics), the batch order is irrelevant, eval forward
    is deterministic, and the train-mode dropout masks are a pure function of (torch seed, forward-call count, position)."""
    cfg = R.default_config(L_in=48, L_out=12, num_nodes=2911, c_in=10, d_emb=12)
    p = R.init_params(cfg, seed=4)
    model = build_model(cfg, p, dev, "per_timestep", precision=precision).eval()
    x, tf, y = R.synthetic_batch(8, 48, 2911, 10, 12, seed=77)
    ei = R.grid_graph()[0].to(dev)
    xd = x.to(dev)
    tfd = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(8, 48, 2911, 4)
    with torch.no_grad():
        full = model(xd, tfd, ei)
        again = model(xd, tfd, ei)
        assert full.shape == (8, 12, 2911, 1) and torch.isfinite(full).all()
        assert torch.equal(full, again)                                   # deterministic
        for b in (0, 3, 7):
            alone = model(xd[b:b + 1], tfd[b:b + 1], ei)
            assert torch.equal(alone[0], full[b]), b                      # sample independence, bit-exact
        perm = torch.tensor([5, 2, 7, 0, 1, 6, 3, 4], device=dev)
        tf_perm = tfd[:, :, 0, :][perm].contiguous().unsqueeze(-2).expand(8, 48, 2911, 4)      # still the train.py:65 view
        shuffled = model(xd[perm], tf_perm, ei)
        assert torch.equal(shuffled, full[perm])                          # batch-order equivariance, bit-exact
        # the same time features materialised per node take the general path (embedding rows rebuilt per graph instead
        # of the temporal embedding folded into the bias): another fp32 association of the same sum
        general = model(xd[perm], tfd[perm], ei)
        # (bf16 mode: a 1e-7 difference in the spatial stage's output is amplified to the bf16 noise floor by the chain
        # of roundings behind it -- tests/parity.py, RTOL_BF16_MODEL)
        assert tfd[perm].stride(2) != 0 and rel_err(general, full[perm]) < (1e-5 if precision == "fp32" else 2e-2)
    from src.model import modules as M_
    model.train()

    def run(seed, call, n=2):
        torch.manual_seed(seed)
        M_._seed_counter[0] = call                                        # mask seed = f(torch seed, forward-call count)
        return model(xd[:n], tfd[:n], ei)
    with torch.no_grad():
        a, b_, c, d_ = run(11, 0), run(11, 0), run(12, 0), run(11, 1)
    assert torch.equal(a, b_) and not torch.equal(a, c) and not torch.equal(a, d_)

    # the full training-mode backward at B = 8: everything behind the spatial stage (55 tensors: split-K slabs and
    # per-block partial rows reduced in a fixed order) is bit-deterministic; the 11 tensors of the spatial stage
    # (embedding tables, GATv2) are accumulated with float atomics (csrc/spatial_bwd.hip) and repeat to 1e-5
    def grads():
        model.zero_grad(set_to_none=True)
        torch.nn.functional.huber_loss(run(11, 0, 8), y.to(dev)).backward()
        return {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
    g1, g2 = grads(), grads()
    assert len(g1) == 66 and all(torch.isfinite(v).all() for v in g1.values())
    spatial = [k for k in g1 if k.startswith(("spatio_temporal_embedding.", "spatial_encoder."))]
    assert len(spatial) == 11
    assert all(torch.equal(g1[k], g2[k]) for k in g1 if k not in spatial), \
        [k for k in g1 if k not in spatial and not torch.equal(g1[k], g2[k])]
    assert all(rel_err(g1[k], g2[k]) < 1e-5 for k in spatial), [(k, rel_err(g1[k], g2[k])) for k in spatial]


@pytest.mark.parametrize("kind", ["no_edges", "irregular"])
def test_spatial_irregular_graphs(dev, kind):
    """Graphs a lat/lon grid never produces: no edges at all (every node sees only its implicit self loop), and a
    random directed multigraph with duplicate edges (kept, PyG semantics), explicit self loops (stripped and re-added
    once), isolated nodes, one high-degree hub and long-range edges (wide LDS windows).  Forward and all gradients
    against the oracle."""
    N, B, L = 150, 2, 3
    cfg = R.default_config(num_nodes=N)
    p = R.init_params(cfg, seed=8)
    x, tf, _ = R.synthetic_batch(B, L, N, cfg["spatial_in_channels_base"], 12, seed=9)
    g = torch.Generator().manual_seed(10)
    if kind == "no_edges":
        ei = torch.zeros(2, 0, dtype=torch.int64)
    else:
        src = torch.randint(0, N, (400,), generator=g)
        dst = torch.randint(0, N, (400,), generator=g)
        dst[dst == 7] = 8                                       # node 7: no in-edges
        hub = torch.stack([torch.arange(40, 100), torch.full((60,), 3)])          # node 3: 60 extra in-edges
        loops = torch.stack([torch.arange(0, 20), torch.arange(0, 20)])           # explicit self loops
        dup = torch.stack([src[:50], dst[:50]])                                    # duplicates
        ei = torch.cat([torch.stack([src, dst]), hub, loops, dup], 1)
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items() if k.startswith((R.P_EMB, R.P_GAT))}
    ref = R.spatial(R.embed(x, tf, pr), ei, pr, 2, None)
    ref_tm = ref.view(L, B, N, 22).permute(1, 0, 2, 3)
    out, ps, names = _run_spatial(p, x, tf, ei, dev, B * L)
    assert_close(out[..., :22], ref_tm)
    gout = torch.randn(B, L, N, 22, generator=torch.Generator().manual_seed(11))
    gref = torch.autograd.grad(ref_tm, [pr[n] for n in names], gout)
    gpad = torch.zeros(B, L, N, 24)
    gpad[..., :22] = gout
    ghip = torch.autograd.grad(out, ps, gpad.to(dev))
    for n, a, b in zip(names, ghip, gref):
        assert_close(a, b, n)


def test_out_of_range_time_index_is_rejected_not_clamped(dev):
    """modules.py:255-258: nn.Embedding raises on an out-of-range index.  The kernel reports it through the device error
    word (IndexError at the next check, no synchronisation added to the step) and poisons every output built from it."""
    import tecmollm
    from src.data.dataset import SlidingWindowSamplerDataset
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=12)
    p = R.init_params(cfg, seed=1)
    model = build_model(cfg, p, dev, "per_timestep").eval()
    x, tf, _ = R.synthetic_batch(2, 16, 12, 6, 12, seed=2)
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev)
    tecmollm.check_device_errors()                                   # clean slate
    with torch.no_grad():
        good = model(x.to(dev), tf.to(dev), ei)
    tecmollm.check_device_errors()
    assert torch.isfinite(good).all()
    for col, bad_value, word in ((2, 13.0, "year"), (0, 12.0, "time-of-day"), (1, -1.0, "day-of-year"), (3, 4.0, "season")):
        tfb = tf.clone()
        tfb[1, 5, :, col] = bad_value                                # one (b, t) graph of sample 1
        with torch.no_grad():
            out = model(x.to(dev), tfb.to(dev), ei)
        with pytest.raises(IndexError, match=word):
            tecmollm.check_device_errors()
        assert torch.isnan(out[1]).all() and torch.isfinite(out[0]).all()     # rejected, not repaired; sample 0 untouched
        tecmollm.check_device_errors()                               # the word was cleared by the raise
    # deferred form: the NEXT forward raises without anybody asking
    tfb = tf.clone()
    tfb[0, 0, :, 2] = 99.0
    with torch.no_grad():
        model(x.to(dev), tfb.to(dev), ei)
        torch.cuda.synchronize()
        with pytest.raises(IndexError):
            model(x.to(dev), tf.to(dev), ei)
    # a resident split validates its time features once, at construction
    X = torch.randn(40, 3, 4, 6)
    Y = torch.randn(40, 3, 4, 12)
    tfeat = torch.stack([torch.randint(0, hi, (40,)) for hi in (12, 366, 13, 4)], -1).float()
    SlidingWindowSamplerDataset.from_tensors(X, Y, tfeat, 16, 12, device=dev)
    tfeat[7, 1] = 366.0
    with pytest.raises(IndexError, match="day-of-year"):
        SlidingWindowSamplerDataset.from_tensors(X, Y, tfeat, 16, 12, device=dev)


def test_unfreezing_a_gpt2_base_weight_is_refused(dev):
    """modules.py:195-203 trains only lora_/ln_/wpe inside GPT-2; the HIP backward forms exactly those gradients, so a
    base weight with requires_grad=True must raise instead of silently receiving no gradient."""
    from tecmollm import TecmError
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=12, llm_layers=1)
    model = build_model(cfg, R.init_params(cfg, seed=1), dev).eval()
    x, tf, _ = R.synthetic_batch(1, 16, 12, 6, 12, seed=2)
    ei = R.grid_graph(3, 4, threshold_km=170.0)[0].to(dev)
    model.llm_backbone.trunk.h[0].mlp.c_fc.weight.requires_grad_(True)
    with pytest.raises(TecmError, match="mlp.c_fc.weight"):
        model(x.to(dev), tf.to(dev), ei)


# ----------------------------------------------------------------------------- the two fused modules on their own
def test_standalone_spatio_temporal_embedding_forward_backward(dev):
    """SpatioTemporalEmbedding.forward with the reference's signature and shapes (modules.py:230-266): bit-exact
    output (index gather + the reference's association of the four temporal sums), table gradients vs autograd of the
    oracle; both the stride-0 expanded time features of train.py:65 and per-node ones."""
    from src.model.modules import SpatioTemporalEmbedding
    B, L, N = 2, 5, 37
    cfg = R.default_config(num_nodes=N)
    p = R.init_params(cfg, seed=3)
    mod = SpatioTemporalEmbedding(16, N, 13)
    mod.load_state_dict({k[len(R.P_EMB):]: v for k, v in p.items() if k.startswith(R.P_EMB)})
    mod = mod.to(dev)
    x, tf, _ = R.synthetic_batch(B, L, N, 6, 12, seed=4)
    g = torch.Generator().manual_seed(5)
    tf_node = torch.stack([torch.randint(0, hi, (B, L, N), generator=g) for hi in (12, 366, 13, 4)], -1).float()
    gout = torch.randn(B, L, N, 22, generator=g)
    for tfc, tfd in ((tf, tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(B, L, N, 4)), (tf_node, tf_node.to(dev))):
        pr = {k: v.clone().requires_grad_(True) for k, v in p.items() if k.startswith(R.P_EMB)}
        ref = R.embed(x, tfc, pr)
        out = mod(x.to(dev), tfd)
        assert out.shape == (B, L, N, 22) and torch.equal(out.cpu(), ref.detach())
        names = [R.P_EMB + f"{n}_embedding.weight" for n in ("node", "tod", "doy", "year", "season")]
        gref = torch.autograd.grad(ref, [pr[n] for n in names], gout)
        ghip = torch.autograd.grad(out, [mod.node_embedding.weight, mod.tod_embedding.weight, mod.doy_embedding.weight,
                                         mod.year_embedding.weight, mod.season_embedding.weight], gout.to(dev))
        for n, a, b in zip(names, ghip, gref):
            assert rel_err(a, b) < 1e-5, n


@pytest.mark.parametrize("mode", ["reference", "per_timestep"])
def test_standalone_spatial_encoder_forward_backward(dev, mode):
    """SpatialEncoder.forward with the reference's signature (modules.py:340-359): x (num_graphs, N, 22) ->
    GATv2Conv output (no residual), parameter gradients vs the oracle; a single-graph edge_index reaches only graph 0
    in the reference's literal mode."""
    from src.model.modules import SpatialEncoder
    G, grid = 7, (9, 15)
    N = grid[0] * grid[1]
    cfg = R.default_config(num_nodes=N)
    p = R.init_params(cfg, seed=6)
    enc = SpatialEncoder(22, 11, 2).eval()
    enc.load_state_dict({k[len("spatial_encoder."):]: v for k, v in p.items() if k.startswith(R.P_GAT)})
    enc = enc.to(dev)
    enc.gat_graphs = mode
    g = torch.Generator().manual_seed(7)
    x = torch.randn(G, N, 22, generator=g)
    ei, _ = R.grid_graph(*grid)
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items() if k.startswith(R.P_GAT)}
    bei = R.batched_edge_index(ei, N, 1 if mode == "reference" else G)
    ref = R.gatv2_conv(x.reshape(-1, 22), bei, pr, 2).view(G, N, 22)
    out = enc(x.to(dev), ei.to(dev))
    assert out.shape == (G, N, 22) and rel_err(out, ref) < TOL and elem_err(out, ref) < 1.0
    names = [R.P_GAT + n for n in ("lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "att", "bias")]
    gout = torch.randn(G, N, 22, generator=g)
    gref = torch.autograd.grad(ref, [pr[n] for n in names], gout)
    ghip = torch.autograd.grad(out, list(enc.params()), gout.to(dev))
    for n, a, b in zip(names, ghip, gref):
        assert_close(a, b, n)
    with pytest.raises(Exception):
        enc(x.to(dev).requires_grad_(True), ei.to(dev)).sum().backward()   # d x is not part of the MI355X path


def test_gatv2_kernel_matches_the_hand_derived_known_answer(dev):
    """The HIP GATv2 kernel against literal numbers derived by hand from Brody et al. eq. 7 and PyG's source -> target
    convention on a 3-node ASYMMETRIC graph (tests/parity.py GAT_KAT_*; the same vectors pin the oracle in
    tests/test_oracle.py): edge direction and the lin_l-on-source assignment are checked by something neither the
    kernel nor the restatement was written from.  Reference call site: modules.py:329-336, :356."""
    from parity import GAT_KAT_WRONG_DIRECTION_1_0, GAT_KAT_WRONG_ROLES_1_0, gat_kat_tensors
    from src.model.modules import SpatialEncoder
    x, ei, p, want = gat_kat_tensors()
    enc = SpatialEncoder(22, 11, 2).eval()
    enc.load_state_dict({k[len("spatial_encoder."):]: v for k, v in p.items()})
    enc = enc.to(dev)
    enc.gat_graphs = "per_timestep"
    G = 5
    out = enc(x.unsqueeze(0).repeat(G, 1, 1).to(dev), ei.to(dev)).cpu()
    for g in range(G):
        torch.testing.assert_close(out[g], want, rtol=0, atol=2e-6)
    assert abs(float(out[0, 1, 0]) - GAT_KAT_WRONG_DIRECTION_1_0) > 0.5
    assert abs(float(out[0, 1, 0]) - GAT_KAT_WRONG_ROLES_1_0) > 1e-2
    enc.gat_graphs = "reference"                      # the reference's literal mode: graph 0 has the edges, the rest self loops
    out = enc(x.unsqueeze(0).repeat(G, 1, 1).to(dev), ei.to(dev)).cpu()
    torch.testing.assert_close(out[0], want, rtol=0, atol=2e-6)
    torch.testing.assert_close(out[1:, :, 0], (x[:, 0] + 0.05).expand(G - 1, 3), rtol=0, atol=1e-6)
