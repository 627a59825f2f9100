"""GPU tests of the gradient with respect to the model's INPUT (csrc/spatial_dx.hip, SpatialFn.backward) and of the attribution
interface built on it (tecmollm/attribute.py), against the CPU oracle with `x.requires_grad_()`.  Bars: the standard fp32
bars of tests/parity.py (`assert_close`); ATOL_RMS_KINK for the full 2911-node graph only (dx passes through the same
lrelu'(x_l[j] + x_r[i]) as the tensors that bar was stated for); RTOL_BF16_MODEL / ATOL_RMS_BF16_MODEL in bf16 mode."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests.input_grad_cases import (GRID_ONE_TILE, GRID_TWO_TILES, GRID_WIDE, asymmetric_edges, grid_edges, oracle_model_dx,
                                    oracle_stage_dx)
from tests.parity import (ATOL_RMS_BF16_MODEL, ATOL_RMS_KINK, RTOL_BF16_MODEL, assert_close, build_model, device_masks,
                          device_rounding, elem_err, rel_err)

pytestmark = pytest.mark.gpu

SPATIAL = [R.P_EMB + f"{n}_embedding.weight" for n in ("node", "tod", "doy", "year", "season")] + \
          [R.P_GAT + n for n in ("lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "att", "bias")]
B_ST, L_ST, SEED_ST = 2, 3, 987654321                       # the stage tests: six graphs


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


_mask_cache = {}


def _gat_masks(name, ei, N, mode):
    """The alpha-dropout multipliers of one training-mode forward of the stage tests, in the oracle's edge order."""
    key = (name, mode)
    if key not in _mask_cache:
        mcfg = dict(R.default_config(num_nodes=N), temporal_seq_len=L_ST, temporal_strides=[1, 1], patch_len=1, llm_layers=0)
        _mask_cache[key] = device_masks(mcfg, B_ST, ei, SEED_ST, mode)["gat"]
    return _mask_cache[key]


def _stage_inputs(N, cin, per_node, seed):
    cfg = R.default_config(num_nodes=N, c_in=cin, d_emb=22 - cin)
    p = {k: v for k, v in R.init_params(cfg, seed=seed).items() if k.startswith((R.P_EMB, R.P_GAT))}
    x, tf, _ = R.synthetic_batch(B_ST, L_ST, N, cin, 12, seed=seed + 1)
    if per_node:                                             # time features that really vary over the nodes
        g = torch.Generator().manual_seed(seed + 2)
        tf = torch.stack([torch.randint(0, hi, (B_ST, L_ST, N), generator=g) for hi in (12, 366, 13, 4)], -1).float()
    gout = torch.randn(B_ST, L_ST, N, 22, generator=torch.Generator().manual_seed(seed + 3))
    return p, x, tf, gout


def _stage_dx(p, x, tf, ei, gout, dev, mode, train, per_node, params_need_grad=False):
    """d x of the fused stage on the device; `tf` is handed over as the stride-0 view of train.py:65 unless per_node."""
    from tecmollm import functions as F_
    from tecmollm import graph
    B, L, N, _ = x.shape
    meta = graph.get(ei.to(dev), N, dev, p[SPATIAL[0]].shape[1])
    ps = [p[n].to(dev).requires_grad_(params_need_grad) for n in SPATIAL]
    tfd = tf.to(dev) if per_node else tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(B, L, N, 4)
    plan = F_.DropPlan(True, 0.1, SEED_ST) if train else F_.DropPlan(False, 0.0, 0)
    xd = x.to(dev).requires_grad_(True)
    out = F_.SpatialFn.apply(xd, tfd, *ps, meta, 2, 1 if mode == "reference" else B * L, plan)
    gpad = torch.zeros(B, L, N, 24)
    gpad[..., :22] = gout
    grads = torch.autograd.grad(out, [xd] + (ps if params_need_grad else []), gpad.to(dev))
    return grads[0], grads[1:]


def _check_stage(name, ei, N, cin, per_node, mode, train, dev, seed):
    p, x, tf, gout = _stage_inputs(N, cin, per_node, seed)
    mult = _gat_masks(name, ei, N, mode) if train else None
    want = oracle_stage_dx(p, x, tf, ei, 1 if mode == "reference" else None, gout, mult)
    got, _ = _stage_dx(p, x, tf, ei, gout, dev, mode, train, per_node)
    assert got.shape == x.shape and torch.isfinite(got).all()
    print(f"{name} cin={cin} per_node={per_node} {mode} train={train}: max-norm {rel_err(got, want):.2e}, "
          f"element-wise {elem_err(got, want):.3f} of the bar")
    assert_close(got, want, "dx")
    return got, want, (p, x, tf, gout)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("mode", ["reference", "per_timestep"])
@pytest.mark.parametrize("per_node", [False, True], ids=["tf_uniform", "tf_per_node"])
@pytest.mark.parametrize("cin", [6, 10])
@pytest.mark.parametrize("grid", [GRID_ONE_TILE, GRID_TWO_TILES, GRID_WIDE], ids=["n12", "n135", "n420_wide"])
def test_stage_dx_matches_oracle(dev, grid, cin, per_node, mode, train):
    """SpatialFn's gradient for x against autograd through the oracle's embed + spatial: one tile, two tiles (sources whose
    targets sit in the other tile), and a window of 346 rows (the forward's first kernel); both graph modes, eval and the
    mirrored alpha-dropout masks, block-uniform and per-node time features, both feature widths.  The eleven parameters do
    not require grad here: the backward launches the input gradient alone."""
    _check_stage(f"{grid[0]}x{grid[1]}", grid_edges(grid), grid[0] * grid[1], cin, per_node, mode, train, dev, seed=21)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("mode", ["reference", "per_timestep"])
def test_stage_dx_on_an_asymmetric_graph(dev, mode, train):
    """Half of the directed edges dropped, explicit self loops in the input, a node without in-edges and one without
    out-edges: a transposed direction, a slot taken from the wrong list or a lost self loop all show here."""
    got, want, (p, x, tf, gout) = _check_stage("asymmetric", asymmetric_edges(), 135, 6, False, mode, train, dev, seed=23)
    if not train and mode == "per_timestep":                # the reversed graph has another gradient: the case can tell
        flipped = oracle_stage_dx(p, x, tf, asymmetric_edges().flip(0), 1 if mode == "reference" else None, gout)
        assert rel_err(flipped, want) > 1e-2


def test_stage_dx_is_bit_reproducible_and_independent_of_the_graph_chunking(dev, monkeypatch):
    """Three runs give equal bits (no float atomics on dx), and so do chunks of 1, 2 and 4 graphs against all 6 at once:
    the workspace holds one chunk, the launcher walks them.  Training mode: the dropout index must not depend on the chunk."""
    ei = asymmetric_edges()
    p, x, tf, gout = _stage_inputs(135, 6, False, 27)
    monkeypatch.delenv("TECM_SPATIAL_DX_GRAPHS", raising=False)
    first, _ = _stage_dx(p, x, tf, ei, gout, dev, "per_timestep", True, False)
    for _ in range(2):
        assert torch.equal(_stage_dx(p, x, tf, ei, gout, dev, "per_timestep", True, False)[0], first)
    for gc in ("1", "2", "4"):
        monkeypatch.setenv("TECM_SPATIAL_DX_GRAPHS", gc)
        assert torch.equal(_stage_dx(p, x, tf, ei, gout, dev, "per_timestep", True, False)[0], first), gc


def test_stage_parameter_gradients_do_not_depend_on_the_input_gradient(dev):
    """The eleven parameter gradients with and without x.requires_grad, eval: the input gradient is a launch of its own and
    touches nothing the parameter backward reads.  The tables are accumulated with float atomics: 1e-5 for all eleven."""
    from tecmollm import functions as F_
    from tecmollm import graph
    ei = grid_edges(GRID_TWO_TILES)
    p, x, tf, gout = _stage_inputs(135, 6, False, 29)
    _, with_dx = _stage_dx(p, x, tf, ei, gout, dev, "per_timestep", False, False, params_need_grad=True)
    meta = graph.get(ei.to(dev), 135, dev, 16)
    ps = [p[n].to(dev).requires_grad_(True) for n in SPATIAL]
    tfd = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(B_ST, L_ST, 135, 4)
    out = F_.SpatialFn.apply(x.to(dev), tfd, *ps, meta, 2, B_ST * L_ST, F_.DropPlan(False, 0.0, 0))
    gpad = torch.zeros(B_ST, L_ST, 135, 24)
    gpad[..., :22] = gout
    without = torch.autograd.grad(out, ps, gpad.to(dev))
    for n, a, b in zip(SPATIAL, with_dx, without):
        assert rel_err(a, b) <= 1e-5, (n, rel_err(a, b))


def test_bad_time_index_gives_nan_rows_and_sets_the_error_word(dev):
    """An out-of-range time index behaves as in the forward: the rows built from it are NaN (here: graph (b = 1, t = 2) and,
    through its edges, nothing else), and the device error word makes the next poll raise IndexError."""
    from tecmollm import devcheck
    ei = grid_edges(GRID_ONE_TILE)
    p, x, tf, gout = _stage_inputs(12, 6, False, 31)
    tf = tf.clone()
    tf[1, 2, :, 1] = 400.0                                  # day of year outside [0, 366)
    got, _ = _stage_dx(p, x, tf, ei, gout, dev, "per_timestep", False, False)
    torch.cuda.synchronize()
    with pytest.raises(IndexError, match="day-of-year"):
        devcheck.check_device_errors(dev)
    bad = torch.isnan(got).flatten(2).any(-1)               # (B, L)
    want = torch.zeros(B_ST, L_ST, dtype=torch.bool)
    want[1, 2] = True
    assert torch.equal(bad.cpu(), want)
    assert torch.isnan(got[1, 2]).all()


# ------------------------------------------------------------------------------------------------ whole model
def _model_case(N_grid, B, mode, train, precision, dev, seed, L_in=16):
    """One Huber step with x.requires_grad on both sides: (dx device, dx oracle, {name: (grad device, grad oracle)})."""
    from src.model import modules as M_
    from tecmollm import functions as F_
    N = N_grid[0] * N_grid[1]
    cfg = R.default_config(L_in=L_in, L_out=12, num_nodes=N, llm_layers=1)
    params = R.init_params(cfg, seed=seed)
    x, tf, y = R.synthetic_batch(B, L_in, N, 6, 12, seed=seed + 100)
    ei = grid_edges(N_grid)
    masks = None
    if train:
        torch.manual_seed(4242 + seed)
        M_._seed_counter[0] = 17                             # make_plan: base = initial_seed + 7919 * (count + 1)
        masks = device_masks(cfg, B, ei, torch.initial_seed() + 7919 * 18, mode)
    q = device_rounding(N) if precision == "bf16" else R.FP32
    dx_ref, grads_ref = oracle_model_dx(cfg, params, x, tf, ei, y, 1 if mode == "reference" else None, masks, q)
    model = build_model(cfg, params, dev, mode, precision=precision)
    model.train(train)
    xd = x.to(dev).requires_grad_(True)
    tfd = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(B, L_in, N, 4)
    F_.HuberFn.apply(model(xd, tfd, ei.to(dev)), y.to(dev), 1.0).backward()
    torch.cuda.synchronize()
    assert xd.grad is not None and xd.grad.shape == x.shape
    named = dict(model.named_parameters())
    return xd.grad, dx_ref, {k: (named[k].grad, g) for k, g in grads_ref.items()}


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("mode", ["reference", "per_timestep"])
@pytest.mark.parametrize("grid", [GRID_ONE_TILE, GRID_TWO_TILES], ids=["n12", "n135"])
def test_model_x_grad_matches_oracle_fp32(dev, grid, mode, train):
    """x.grad of the Huber loss, L_in = 16, one GPT-2 layer, B = 2.  (fp32 oracle against the same oracle in fp64 at these
    shapes: max-norm 1e-6, worst element 1 % of the bar.)"""
    dx, dx_ref, grads = _model_case(grid, 2, mode, train, "fp32", dev, seed=41)
    print(f"dx max-norm {rel_err(dx, dx_ref):.2e}, element-wise {elem_err(dx, dx_ref):.3f} of the bar")
    assert_close(dx, dx_ref, "x.grad")
    assert set(SPATIAL) <= set(grads) and all(g is not None for g, _ in grads.values())


def test_model_x_grad_matches_oracle_fp32_full_graph(dev):
    """N = 2911 (26 tiles), B = 1, every graph with edges.  The one case with ATOL_RMS_KINK: dx passes through the same
    lrelu'(x_l[j] + x_r[i]) as the tensors that bar exists for (tests/parity.py)."""
    dx, dx_ref, _ = _model_case((41, 71, 150.0), 1, "per_timestep", False, "fp32", dev, seed=43)
    print(f"dx max-norm {rel_err(dx, dx_ref):.2e}, element-wise {elem_err(dx, dx_ref):.3f} of the standard bar, "
          f"{elem_err(dx, dx_ref, atol_rms=ATOL_RMS_KINK):.3f} of the kink bar")
    assert_close(dx, dx_ref, "x.grad", atol_rms=ATOL_RMS_KINK)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_model_x_grad_matches_oracle_bf16(dev, train):
    """bf16 mode, N = 135, against the bf16-emulating oracle with the device's storage policy; the model-level bf16 bars."""
    dx, dx_ref, grads = _model_case(GRID_TWO_TILES, 2, "per_timestep", train, "bf16", dev, seed=47)
    worst = max((elem_err(g, gr, RTOL_BF16_MODEL, ATOL_RMS_BF16_MODEL), k) for k, (g, gr) in grads.items() if gr.abs().max() > 0)
    print(f"dx max-norm {rel_err(dx, dx_ref):.2e}, element-wise {elem_err(dx, dx_ref, RTOL_BF16_MODEL, ATOL_RMS_BF16_MODEL):.3f} "
          f"of the bar; worst parameter gradient {worst[0]:.3f} of the bar ({worst[1]})")
    assert_close(dx, dx_ref, "x.grad", rtol=RTOL_BF16_MODEL, atol_rms=ATOL_RMS_BF16_MODEL)


def _model_and_batch(dev, grid=GRID_ONE_TILE, B=2, seed=51, mode="per_timestep"):
    N = grid[0] * grid[1]
    cfg = R.default_config(L_in=16, L_out=12, num_nodes=N, llm_layers=1)
    params = R.init_params(cfg, seed=seed)
    x, tf, y = R.synthetic_batch(B, 16, N, 6, 12, seed=seed + 100)
    ei = grid_edges(grid)
    model = build_model(cfg, params, dev, mode, precision="fp32").eval()
    tfd = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(B, 16, N, 4)
    return cfg, params, model, (x, tf, y, ei), (x.to(dev), tfd, y.to(dev), ei.to(dev))


def test_model_x_grad_is_reproducible_and_leaves_the_parameter_gradients_alone(dev):
    """fp32 eval, N = 135: three backward runs give torch.equal x.grad; with and without x.requires_grad the parameter
    gradients (54 tensors with one GPT-2 layer, 66 with three) outside the spatial stage are bit-identical, the eleven of the spatial stage (tables by float atomics) agree
    to 1e-5."""
    from tecmollm import functions as F_
    _, _, model, _, (xd, tfd, yd, eid) = _model_and_batch(dev, GRID_TWO_TILES)

    def step(need_dx):
        model.zero_grad(set_to_none=True)
        xi = xd.clone().requires_grad_(need_dx)
        F_.HuberFn.apply(model(xi, tfd, eid), yd, 1.0).backward()
        return xi.grad, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    dx0, g_with = step(True)
    for _ in range(2):
        assert torch.equal(step(True)[0], dx0)
    none, g_without = step(False)
    assert none is None and g_with.keys() == g_without.keys() and set(SPATIAL) <= set(g_with)
    for k in g_with:
        if k in SPATIAL:
            assert rel_err(g_with[k], g_without[k]) <= 1e-5, k
        else:
            assert torch.equal(g_with[k], g_without[k]), k


# ------------------------------------------------------------------------------------------------ attribution
def _oracle_F(cfg, params, x, tf, ei, horizons, nodes):
    out = R.forward(x, tf, ei, params, cfg, None)[..., 0]
    if horizons is not None:
        out = out[:, horizons]
    if nodes is not None:
        out = out[:, :, nodes]
    return out.sum(dim=(1, 2))


def test_input_gradient_selections_and_loss_match_oracle(dev):
    import tecmollm
    cfg, params, model, (x, tf, y, ei), (xd, tfd, yd, eid) = _model_and_batch(dev)
    flags = [p.requires_grad for p in model.parameters()]
    for horizons, nodes in ((None, None), ([0, 3, 11], None), (None, [1, 5, 7]), ([2], [0, 11])):
        xr = x.clone().requires_grad_(True)
        want = torch.autograd.grad(_oracle_F(cfg, params, xr, tf, ei, horizons, nodes).sum(), xr)[0]
        got = tecmollm.input_gradient(model, xd, tfd, eid, horizons=horizons, nodes=nodes)
        assert_close(got, want, f"input_gradient(horizons={horizons}, nodes={nodes})")
    xr = x.clone().requires_grad_(True)
    want = torch.autograd.grad(R.huber(R.forward(xr, tf, ei, params, cfg, None), y), xr)[0]
    assert_close(tecmollm.input_gradient(model, xd, tfd, eid, y=yd), want, "input_gradient(y)")
    assert [p.requires_grad for p in model.parameters()] == flags and not model.training
    assert all(p.grad is None for p in model.parameters()) and not xd.requires_grad


def test_integrated_gradients_match_the_oracle_rule_and_close_the_completeness_gap(dev):
    """The midpoint rule with the same `steps` on the oracle; |delta| <= the oracle's own |delta| + 1e-3 |F(x) - F(x0)|."""
    import tecmollm
    cfg, params, model, (x, tf, y, ei), (xd, tfd, yd, eid) = _model_and_batch(dev)
    steps, horizons, nodes = 8, [0, 5], None
    x0 = 0.25 * torch.ones_like(x)
    for base, based in ((None, None), (x0, x0.to(dev))):
        b = torch.zeros_like(x) if base is None else base
        acc = torch.zeros_like(x)
        for k in range(steps):
            xr = (b + ((k + 0.5) / steps) * (x - b)).requires_grad_(True)
            acc += torch.autograd.grad(_oracle_F(cfg, params, xr, tf, ei, horizons, nodes).sum(), xr)[0]
        want = (x - b) * (acc / steps)
        with torch.no_grad():
            dF = _oracle_F(cfg, params, x, tf, ei, horizons, nodes) - _oracle_F(cfg, params, b, tf, ei, horizons, nodes)
        delta_ref = want.sum(dim=(1, 2, 3)) - dF
        model.train()                                        # integrated_gradients runs in eval mode and restores this
        attr, delta = tecmollm.integrated_gradients(model, xd, tfd, eid, baseline=based, steps=steps, horizons=horizons,
                                                    nodes=nodes)
        assert model.training and attr.shape == x.shape and delta.shape == (x.shape[0],)
        model.eval()
        print(f"IG max-norm {rel_err(attr, want):.2e}; delta {delta.tolist()} oracle {delta_ref.tolist()} dF {dF.tolist()}")
        assert_close(attr, want, "integrated gradients")
        assert (delta.cpu().abs() <= delta_ref.abs() + 1e-3 * dF.abs()).all()
    maps = tecmollm.attribution_maps(attr, ["tec", "f107", "kp", "ap", "dst", "ae"])
    assert maps["lag_channel"].shape == (16, 6) and maps["node_channel"].shape == (12, 6) and maps["channel"].shape == (6,)
    total = attr.abs().sum() / attr.shape[0]
    for k in ("lag_channel", "node_channel", "channel"):
        assert abs(float(maps[k].sum()) - float(total)) <= 1e-5 * float(total)
    assert torch.allclose(maps["lag_channel"].sum(0), maps["channel"], rtol=1e-5)


def test_write_attributions_round_trip_from_the_device(dev, tmp_path):
    import tecmollm
    attr = torch.randn(2, 4, 12, 6, generator=torch.Generator().manual_seed(3)).to(dev)
    maps = tecmollm.attribution_maps(attr)
    z = np.load(tecmollm.write_attributions(maps, str(tmp_path), grid=(3, 4))["npz"])
    assert z["node_channel"].shape == (3, 4, 6) and z["lag_channel"].shape == (4, 6)
    assert np.array_equal(z["channel"], maps["channel"].cpu().numpy())
    assert np.array_equal(z["node_channel"].reshape(12, 6), maps["node_channel"].cpu().numpy())
