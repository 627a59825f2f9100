"""Parity helpers shared by the GPU tests, `__graft_entry__.smoke()` and `bench.py`'s cpu_baseline leg.
Lives under tests/ because it imports the oracle (test infrastructure); the product package never does."""
from __future__ import annotations

import os
import sys
from typing import Dict, Optional, Tuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import ref_cpu as R  # noqa: E402

RTOL = 1e-3          # north star: "within 1e-3 rel fp32"
# Absolute slack of the element-wise bar, as a fraction of the oracle tensor's RMS: |a-b| <= RTOL*|b| + ATOL_RMS*rms(b).
ATOL_RMS = 5e-4
# The ONE documented exception, applied only where a test passes `kink=True` (the full 2911-node graph): GATv2's
# LeakyReLU has a kink -- when a sum x_l[j,c] + x_r[i,c] lands within rounding distance of 0 the two sides can see
# opposite signs, lrelu' jumps between 0.2 and 1, and ONE term of a gradient sum changes (observed at N = 2911, 48
# graphs: two neighbouring rows of the node-table gradient off by 1.8e-3 of its RMS, every other row below 2e-5;
# tools/diag_parity.py; train mode, same size: one element of d lin_r.weight at 5.4e-4 of its RMS).  Only the tensors
# whose gradient passes through lrelu'(x_l[j] + x_r[i]) -- the embedding tables and the two GATv2 input transforms -- get
# the wider absolute term; `att`, the output bias and everything downstream of the spatial stage do not.
ATOL_RMS_KINK = 5e-3
KINK_TENSORS = tuple(f"spatio_temporal_embedding.{n}_embedding.weight" for n in ("node", "tod", "doy", "year", "season")) + \
    tuple(f"spatial_encoder.gat_conv.lin_{s}.{w}" for s in ("l", "r") for w in ("weight", "bias"))

# bf16 mode (BASELINE configs[2]) against the bf16-EMULATING oracle (ref_cpu.BF16: the same operand roundings in the
# forward and in the backward contractions).  What is left between the two sides is fp32 summation order PLUS
# rounding flips: a value that differs by one fp32 ulp between the sides can round to a different bf16 neighbour, a
# 2^-9 = 2e-3 relative jump of ONE operand element of the next contraction.  Sums over thousands of such elements
# average the flips out (parameter gradients), single activations do not, hence a bar of 1e-2 relative +
# 1e-2 * rms(b) absolute -- ten times the fp32 bar, ten times tighter than bf16 against the fp32 oracle (8e-2).
RTOL_BF16 = 1e-2
ATOL_RMS_BF16 = 1e-2
# The bar above holds for ONE stage fed identical inputs on both sides (tests/test_gpu_bf16_model.py, stage tests).  It
# cannot hold through the whole model, and no implementation could make it: a relative deviation eps in front of a bf16
# rounding comes out as sqrt(ulp_bf16 * eps) behind it (a flip of probability eps/ulp and size ulp; ulp = 2^-8), so
# 1e-6 (fp32 summation order) -> 6e-5 -> 5e-4 -> 1.4e-3 -> ... converges to the bf16 quantisation noise itself after a
# handful of chained contractions, whatever the starting point (measured stage by stage: tools/diag_bf16.py,
# profiles/r03_bf16_stage_deviation.md).  The model-level statement is therefore (i) fixed bars at the scale of that
# noise floor -- max-norm 2e-2, element-wise 2e-2*|b| + 6e-2*rms(b) (measured worst case over all tests: 1.3e-2 and
# 5.0e-2, on gradients that are sums over only B*T*N = 120 rows), against 8e-2 for bf16 vs the fp32 oracle -- and (ii) the self-calibrated test: the device is as close to the oracle as the oracle is to ITSELF when its
# inputs are perturbed by the fp32-mode deviation between the two implementations (1e-6).
RTOL_BF16_MODEL = 2e-2
ATOL_RMS_BF16_MODEL = 6e-2
# The 40-SEQUENCE test problems (B = 2 x N = 20: 120 tokens, every parameter gradient a sum over 120-1 920 rows) sit ON that
# noise floor, and which tensor is worst moves with the data / mask seed.  Round 5 (new dropout-mask hash, so every
# realisation changed) measured 20 train-mode steps (L_in = 48 and 96, seeds 31..40, profiles/r05_bf16_seed_sweep.txt):
#   element-wise bar, worst tensor per run: 0.91 .. 1.46 of the standard bar (lora_B 11 times, a conv weight 6 times, an
#     embedding table, the patch projection, lin_r once each -- no tensor is worst systematically);
#   max-norm, tensors outside the GATv2 stage: 1.2e-2 .. 2.05e-2;  GATv2 stage (att, bias, lin_l / lin_r: their gradients pass
#     through LeakyReLU'(x_l[j] + x_r[i]), a 0.2 <-> 1 jump wherever bf16-noise-sized differences flip a sign): up to 3.4e-2.
# These problems therefore get ONE stated set of wider bars (`assert_parity(small40=True)`), nothing else does: N = 135 and
# N = 2911 keep the standard bars, and the self-calibrated test (test_gpu_bf16_model.py) is the noise-independent statement.
SMALL40_ELEM_SCALE = 1.6
SMALL40_RTOL = 2.5e-2
SMALL40_RTOL_GAT = 5e-2
GAT_TENSORS = KINK_TENSORS[-4:] + ("spatial_encoder.gat_conv.att", "spatial_encoder.gat_conv.bias")
# ... and the 24-SEQUENCE problems of the configuration sweep (B = 2 x N = 12: 72 token rows at L_in = 48;
# tests/test_gpu_config_sweep.py) sit higher still: 32 bf16 steps over 16 configurations (profiles/r05_config_sweep.txt) --
# worst element per run 0.87 .. 1.56 of the standard bar (round 4, other masks: 0.86 .. 1.94), max-norm 1.2e-2 .. 2.3e-2
# (round 4: .. 3.0e-2).  `assert_parity(small24=True)`; fp32 stays on the standard bars in every configuration (<= 0.05).
SMALL24_ELEM_SCALE = 2.0
SMALL24_RTOL = 3e-2


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """max|a-b| / max|b|  (b = oracle): the global, max-norm relative error."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def elem_err(a: torch.Tensor, b: torch.Tensor, rtol: float = RTOL, atol_rms: float = ATOL_RMS) -> float:
    """Element-wise bar: max over elements of |a-b| / (rtol*|b| + atol), atol = atol_rms * rms(non-zero entries of b).
    A value < 1 means EVERY element satisfies |a-b| <= rtol*|b| + atol (the torch.allclose form with the absolute
    term tied to the tensor's own scale), so a small entry that is wrong by 100 % fails even when the tensor's
    largest entry hides it from `rel_err`.  b = oracle."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    nz = int((b != 0).sum())
    if nz == 0:
        return 0.0 if float((a - b).abs().max()) == 0.0 else float("inf")
    rms = float((b.pow(2).sum() / nz).sqrt())          # RMS of the entries that are used: rows of an embedding / position
    #                                                     table no sample touches have an exactly-zero gradient on both sides
    return float(((a - b).abs() / (rtol * b.abs() + atol_rms * rms)).max())


def l2_rel(a: torch.Tensor, b: torch.Tensor) -> float:
    """||a-b||_2 / ||b||_2  (b = oracle)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def assert_close(a: torch.Tensor, b: torch.Tensor, what: str = "", rtol: float = RTOL, atol_rms: float = ATOL_RMS) -> None:
    """Stage-level bar: max-norm relative error AND the element-wise bar (b = oracle / golden)."""
    r, e = rel_err(a, b), elem_err(a, b, rtol, atol_rms)
    assert r < rtol and e < 1.0, f"{what}: max-norm rel {r:.3e} (bar {rtol}), element-wise {e:.3f} of the bar"


def build_model(cfg: dict, params: Dict[str, torch.Tensor], device, gat_graphs: str = "reference",
                precision: Optional[str] = None):
    """TEC_MoLLM (HIP path) carrying exactly the oracle's parameters (strict state-dict load)."""
    from src.model.tec_mollm import TEC_MoLLM
    mc = dict(cfg)
    mc.update(gat_graphs=gat_graphs, include_wte=False, load_pretrained_gpt2=False)
    if precision is not None:
        mc["precision"] = precision
    model = TEC_MoLLM(mc)
    missing, unexpected = model.load_state_dict(params, strict=True), None
    del missing, unexpected
    return model.to(device)


def device_rounding(num_nodes: int) -> "R.Rounding":
    """The bf16-emulating oracle with the DEVICE's storage policy for the conv-block tensors handed in (which of them are
    bf16 tensors in HBM for a given sequence length: tecmollm.functions.conv_storage_policy, the same two functions
    ConvBlockFn calls).  R.BF16 alone = autocast's semantics (always bf16); the two differ at L_in = 336 only."""
    from tecmollm import functions as F_
    return R.BF16.with_conv_policy(F_.conv_storage_policy(num_nodes))


def oracle_step(cfg, params, x, tf, ei, y, graphs_with_edges,
                masks=None, q: "R.Rounding" = R.FP32) -> Tuple[torch.Tensor, torch.Tensor, Dict[str, torch.Tensor]]:
    """CPU oracle forward + Huber loss + autograd backward.  Returns (out, loss, grads of trainable params).
    q = R.BF16: the bf16-emulating oracle (operand roundings of the forward and backward contractions)."""
    p = {k: v.clone().requires_grad_(R.is_trainable(k)) for k, v in params.items()}
    out = R.forward(x, tf, ei, p, cfg, graphs_with_edges, q=q, masks=masks)
    loss = R.huber(out, y)
    names = [k for k, v in p.items() if v.requires_grad]
    grads = torch.autograd.grad(loss, [p[k] for k in names], allow_unused=True)
    return out.detach(), loss.detach(), {k: (g if g is not None else torch.zeros_like(p[k])) for k, g in zip(names, grads)}


# ------------------------------------------------------------------------------------ mirrored dropout masks
def _tm_to_seq(m: np.ndarray, B: int, T: int, N: int) -> torch.Tensor:
    """(B*T*N, D) time-major rows m = (b*T + t)*N + n  ->  the oracle's (S = B*N, T, D) with s = b*N + n."""
    D = m.shape[1]
    return torch.from_numpy(np.ascontiguousarray(m.reshape(B, T, N, D).transpose(0, 2, 1, 3).reshape(B * N, T, D)))


def device_masks(cfg: dict, B: int, ei: torch.Tensor, base_seed: int, gat_graphs: str, p: float = 0.1) -> dict:
    """The dropout multipliers (0 | 1/(1-p)) the HIP path applies in ONE training-mode forward whose plan has
    `base_seed`, at every site of the reference, laid out the way oracle.ref_cpu.forward(masks=...) wants them.
    Built from tecmollm/rng.py (the bit-for-bit NumPy mirror of csrc/common.h:tecm_hash24) and the site / index
    conventions of tecmollm/functions.py:
        seed(site) = splitmix64(base_seed * 1000003 + site);   idx = logical_row * ld + col
    GATv2 alpha: row = (t*B + b)*N + i, idx = (row*H + head)*(max_deg + 1) + slot, slot = position of the edge in the
    target's in-edge list (self loops removed, given order kept), the implicit self loop last."""
    from tecmollm import functions as F_
    from tecmollm import graph as G_
    from tecmollm import ops, rng
    N, L = cfg["num_nodes"], cfg["temporal_seq_len"]
    H = cfg["spatial_heads"]
    D = cfg["d_llm"]
    T = (L // (cfg["temporal_strides"][0] * cfg["temporal_strides"][1])) // cfg["patch_len"]
    S = B * N
    Hd = (D * T) // 4
    n_layers = cfg["llm_layers"]

    def seed(site):
        return ops.splitmix64(base_seed * 1000003 + site)

    def rows(site, nrows, ncols, ld=None):
        ld = ncols if ld is None else ld
        idx = (np.arange(nrows, dtype=np.uint64)[:, None] * np.uint64(ld) + np.arange(ncols, dtype=np.uint64)[None, :])
        return rng.keep_mult(seed(site), idx, p)

    masks = {}
    # ---- GATv2 attention coefficients (modules.py:333)
    ein = ei.numpy()
    rowptr, colidx = G_.csr_by_target(ein, N)
    deg = np.diff(rowptr).astype(np.int64)
    ld = int(deg.max() if deg.size else 0) + 1
    Gtot = L * B
    Gedges = 1 if gat_graphs == "reference" else Gtot
    src, dst = ein[0].astype(np.int64), ein[1].astype(np.int64)
    nonself = src != dst
    # slot of every given non-self edge inside its target's list (stable order)
    order = np.argsort(dst[nonself], kind="stable")
    slot_sorted = np.arange(order.size, dtype=np.int64) - np.repeat(rowptr[:-1].astype(np.int64), deg)
    slot = np.empty(order.size, dtype=np.int64)
    slot[order] = slot_sorted
    d_ns = dst[nonself]
    # oracle edge order: batched_edge_index -> (graph g, edge e) at g*E + e, self loops of the INPUT removed, then one
    # self loop per row 0..M-1
    g_ids = np.arange(Gedges, dtype=np.int64)
    row_e = (g_ids[:, None] * N + d_ns[None, :]).reshape(-1)
    slot_e = np.tile(slot, Gedges)
    M = Gtot * N
    row_l = np.arange(M, dtype=np.int64)
    node_l = row_l % N
    slot_l = np.where(row_l // N < Gedges, deg[node_l], 0)
    row_all = np.concatenate([row_e, row_l]).astype(np.uint64)
    slot_all = np.concatenate([slot_e, slot_l]).astype(np.uint64)
    hh = np.arange(H, dtype=np.uint64)[None, :]
    idx = (row_all[:, None] * np.uint64(H) + hh) * np.uint64(ld) + slot_all[:, None]
    masks["gat"] = torch.from_numpy(rng.keep_mult(seed(F_.SITE_GAT), idx, p))
    # ---- GPT-2 front end and blocks (time-major rows)
    Mtok = B * T * N
    masks["embd"] = _tm_to_seq(rows(F_.SITE_EMBD, Mtok, D), B, T, N)
    KE = D + F_.LORA_R
    for i in range(n_layers):
        masks[f"lora{i}"] = _tm_to_seq(rows(F_.site_lora(i), Mtok, D, ld=KE), B, T, N)
        aidx = np.arange(S * F_.GPT_HEADS * T * T, dtype=np.uint64)
        masks[f"attn{i}"] = torch.from_numpy(rng.keep_mult(seed(F_.site_attn(i)), aidx, p)).view(S, F_.GPT_HEADS, T, T)
        masks[f"res1_{i}"] = _tm_to_seq(rows(F_.site_res1(i), Mtok, D), B, T, N)
        masks[f"res2_{i}"] = _tm_to_seq(rows(F_.site_res2(i), Mtok, D), B, T, N)
    masks["post"] = _tm_to_seq(rows(F_.SITE_POST, Mtok, D), B, T, N)
    masks["head"] = torch.from_numpy(rows(F_.SITE_HEAD, S, Hd))
    return masks


def compare_forward_backward(cfg: dict, B: int, grid: Tuple[int, int], threshold_km: float = 150.0,
                             gat_graphs: str = "reference", seed: int = 0, use_fused_huber: bool = True,
                             device: Optional[str] = None, train: bool = False, precision: str = "fp32") -> dict:
    """Run the same seeded step through the CPU oracle and the HIP model and report the errors of the forward output,
    the loss and every trainable gradient: `*_rel` = max-norm relative error, `*_elem` = the element-wise bar
    (`elem_err`, < 1 passes).  train=False: eval mode (dropout off).  train=True: training mode, every dropout site of
    the reference active (p = 0.1); the oracle receives the NumPy mirror of the device's counter-based masks
    (`device_masks`), so both sides drop exactly the same elements.
    precision="bf16": the model runs its bf16 mode (BASELINE configs[2]) and the oracle its bf16 emulation (R.BF16);
    the element-wise numbers are then relative to (RTOL_BF16_MODEL, ATOL_RMS_BF16_MODEL)."""
    from src.model import modules as M_
    from tecmollm import functions as F_
    device = device or "cuda"
    N = grid[0] * grid[1]
    assert N == cfg["num_nodes"]
    params = R.init_params(cfg, seed=seed)
    x, tf, y = R.synthetic_batch(B, cfg["temporal_seq_len"], N, cfg["spatial_in_channels_base"],
                                 cfg["prediction_horizon"], seed=seed + 100)
    ei, ew = R.grid_graph(grid[0], grid[1], threshold_km=threshold_km)
    gwe = 1 if gat_graphs == "reference" else None
    masks = None
    if train:
        torch.manual_seed(4242 + seed)
        M_._seed_counter[0] = 17                                  # make_plan: base = initial_seed + 7919 * (count + 1)
        base_seed = torch.initial_seed() + 7919 * 18
        masks = device_masks(cfg, B, ei, base_seed, gat_graphs)
    assert precision in ("fp32", "bf16")
    b16 = precision == "bf16"
    rtol, atol = (RTOL_BF16_MODEL, ATOL_RMS_BF16_MODEL) if b16 else (RTOL, ATOL_RMS)
    out_ref, loss_ref, grads_ref = oracle_step(cfg, params, x, tf, ei, y, gwe, masks, q=device_rounding(N) if b16 else R.FP32)

    model = build_model(cfg, params, device, gat_graphs, precision=precision)
    model.train(train)
    xd, yd = x.to(device), y.to(device)
    tfd = tf[:, :, 0, :].contiguous().to(device).unsqueeze(-2).expand(B, cfg["temporal_seq_len"], N, 4)
    eid, ewd = ei.to(device), ew.to(device)
    out = model(xd, tfd, eid, ewd)
    loss = F_.HuberFn.apply(out, yd, 1.0) if use_fused_huber else torch.nn.functional.huber_loss(out, yd, delta=1.0)
    loss.backward()
    torch.cuda.synchronize()
    res = {"fwd_rel": rel_err(out, out_ref), "fwd_elem": elem_err(out, out_ref, rtol, atol), "fwd_l2": l2_rel(out, out_ref),
           "loss_rel": abs(loss.item() - loss_ref.item()) / abs(loss_ref.item()), "precision": precision}
    worst, worst_name = 0.0, ""
    worst_e, worst_e_name = 0.0, ""
    worst_k, worst_k_name = 0.0, ""
    per = {}
    named = dict(model.named_parameters())
    for k, gref in grads_ref.items():
        g = named[k].grad
        assert g is not None, f"no gradient for trainable parameter {k}"
        nz = gref.abs().max() > 0
        e = rel_err(g, gref) if nz else float(g.abs().max())
        ee = elem_err(g, gref, rtol, atol) if nz else float(g.abs().max())
        per[k] = (e, ee, l2_rel(g, gref) if nz else 0.0)
        if e > worst:
            worst, worst_name = e, k
        if k in KINK_TENSORS and not b16:            # judged separately: `assert_parity(kink=True)` widens only these
            ek = elem_err(g, gref, rtol, ATOL_RMS_KINK) if nz else float(g.abs().max())
            if ek > worst_k:
                worst_k, worst_k_name = ek, k
            res.setdefault("kink_elem_tight", {})[k] = ee
            continue
        if ee > worst_e:
            worst_e, worst_e_name = ee, k
    frozen_with_grad = [k for k, p in named.items() if not R.is_trainable(k) and p.grad is not None]
    res.update(grad_rel_max=worst, grad_worst=worst_name, grad_elem_max=worst_e, grad_elem_worst=worst_e_name,
               kink_elem_max=worst_k, kink_elem_worst=worst_k_name,
               n_grads=len(per), frozen_with_grad=frozen_with_grad)
    res["per_param"] = per
    return res


def batch_vs_single_sample_grads(cfg: dict, B: int, grid: Tuple[int, int], seed: int, precision: str = "fp32",
                                 device: str = "cuda") -> Dict[str, Tuple[float, float]]:
    """Eval-mode gradients of ONE B-sample step (Huber, mean) against the mean of the B single-sample steps' gradients of
    the same model on the same samples (accumulated in float64): {trainable tensor: (max-norm rel, elem_err(rtol=1e-4,
    atol_rms=1e-5))}.  The mean loss of the batch is the mean of the per-sample losses, the forward is per-sample
    bit-exact, and the batch's loss gradient is the single-sample one times 1/B (a power of two for B = 8, so it commutes
    with every bf16 rounding): what may differ is the fp32 summation order of the reductions over rows -- weight
    gradients, split-K slabs, partial rows of the spatial stage and its atomics -- and every shape-keyed choice the batch
    makes (tile heights, split-K counts, graph chunks) that the single-sample step, checked against the oracle, does not."""
    N = grid[0] * grid[1]
    assert N == cfg["num_nodes"]
    L = cfg["temporal_seq_len"]
    model = build_model(cfg, R.init_params(cfg, seed=seed), device, "per_timestep", precision=precision).eval()
    x, tf, y = R.synthetic_batch(B, L, N, cfg["spatial_in_channels_base"], cfg["prediction_horizon"], seed=seed + 100)
    ei = R.grid_graph(grid[0], grid[1])[0].to(device)
    xd, yd = x.to(device), y.to(device)
    tfd = tf[:, :, 0, :].contiguous().to(device).unsqueeze(-2).expand(B, L, N, 4)

    def grads(b0, b1):
        model.zero_grad(set_to_none=True)
        torch.nn.functional.huber_loss(model(xd[b0:b1], tfd[b0:b1], ei), yd[b0:b1]).backward()
        return {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    batch = {k: g.clone() for k, g in grads(0, B).items()}
    acc = {k: torch.zeros_like(g, dtype=torch.float64) for k, g in batch.items()}
    for b in range(B):
        one = grads(b, b + 1)
        assert one.keys() == acc.keys(), sorted(one.keys() ^ acc.keys())
        for k, g in one.items():
            acc[k] += g.double()
    model.zero_grad(set_to_none=True)
    assert all(torch.isfinite(g).all() for g in batch.values())
    return {k: (rel_err(batch[k], acc[k] / B), elem_err(batch[k], acc[k] / B, rtol=1e-4, atol_rms=1e-5)) for k in batch}


def assert_batch_equals_mean_of_samples(errs: Dict[str, Tuple[float, float]], n_grads: int = 66) -> None:
    """The bar of `batch_vs_single_sample_grads`: every trainable gradient within 1e-5 in the max norm (the bar the suite
    uses for the spatial stage's atomics) and element-wise |a-b| <= 1e-4*|b| + 1e-5*rms(b)."""
    worst = max(errs.items(), key=lambda kv: kv[1][0])
    worst_e = max(errs.items(), key=lambda kv: kv[1][1])
    print(f"batch vs mean of samples: max-norm {worst[1][0]:.2e} ({worst[0]}), element-wise {worst_e[1][1]:.3f} of the "
          f"bar ({worst_e[0]})")
    assert len(errs) == n_grads, sorted(errs)
    bad = {k: v for k, v in errs.items() if not (v[0] <= 1e-5 and v[1] < 1.0)}
    assert not bad, bad


def assert_parity(res: dict, tol: Optional[float] = None, kink: bool = False, elem_scale: Optional[dict] = None,
                  small40: bool = False, small24: bool = False) -> None:
    """The bar of every full-step test.  fp32: forward, loss and all gradients within 1e-3 in the max norm AND
    element-wise |a-b| <= 1e-3*|b| + 5e-4*rms(b).  kink=True (full-size graph only): the tensors of KINK_TENSORS get
    the absolute term ATOL_RMS_KINK; without it they meet the same bar as everything else.
    bf16 (res["precision"]): the same two bars at RTOL_BF16_MODEL / ATOL_RMS_BF16_MODEL against the bf16-emulating
    oracle (why not tighter: see the constants).  elem_scale = {tensor name: factor}: the element-wise bar of the named
    gradient tensors times that factor, everything else unchanged.  small40=True (bf16, the 40-sequence problems only): the
    SMALL40_* bars above -- element-wise x1.6 for every gradient, max-norm 2.5e-2 (GATv2-stage tensors 5e-2); small24=True
    (the 24-sequence problems of the configuration sweep): x2.0 and 3e-2."""
    b16 = res.get("precision") == "bf16"
    tol = tol if tol is not None else (RTOL_BF16_MODEL if b16 else RTOL)
    brief = {k: v for k, v in res.items() if k != "per_param"}
    assert res["fwd_rel"] < tol and res["loss_rel"] < tol, brief
    if small40 or small24:
        assert b16, "small40 / small24 are bf16-mode bars"
        rt, es = (SMALL24_RTOL, SMALL24_ELEM_SCALE) if small24 else (SMALL40_RTOL, SMALL40_ELEM_SCALE)
        for k, (e, _, _) in res["per_param"].items():
            assert e < (SMALL40_RTOL_GAT if k in GAT_TENSORS else rt), (k, e, brief)
        elem_scale = dict({"*": es}, **(elem_scale or {}))
    else:
        assert res["grad_rel_max"] < tol, brief
    assert res["fwd_elem"] < 1.0, brief
    if elem_scale:              # named tensors whose element-wise bar a test widens by a stated factor (and says why)
        for k, (_, ee, _) in res["per_param"].items():
            if not (k in KINK_TENSORS and not b16):
                assert ee < elem_scale.get(k, elem_scale.get("*", 1.0)), (k, ee, brief)
    else:
        assert res["grad_elem_max"] < 1.0, brief
    if kink:
        assert res["kink_elem_max"] < 1.0, brief
    else:
        assert all(v < 1.0 for v in res.get("kink_elem_tight", {}).values()), brief
    assert res["frozen_with_grad"] == [], brief


# --------------------------------------------------------------------------------------------------------------------
# GATv2Conv known-answer vectors, derived BY HAND from Brody et al. 2021 eq. 7 and PyG's conventions (edge_index[0] = source j,
# edge_index[1] = target i, messages flow source -> target; lin_l transforms the SOURCE row and is what gets aggregated,
# lin_r transforms the TARGET row; e_ij = att . LeakyReLU_0.2(x_l[j] + x_r[i]); softmax over the sources j of one target
# i, self loop included; out_i = sum_j alpha_ij x_l[j] + bias).  Literal numbers, no code shared with oracle/ref_cpu.py or
# the kernels.  The graph is ASYMMETRIC on purpose: a transposed edge direction or swapped lin_l / lin_r roles give
# different numbers at every node (the reference's own graph is symmetric and could not tell).
#
#   3 nodes, 22 channels, heads = 2 x 11.  Only input features 0 and 1 are non-zero:
#       x0 = (1, 2), x1 = (-1, 0.5), x2 = (0.5, -1.5)
#   lin_l: out[0]  = in[0]              (head 0, channel 0)      lin_r: out[0]  = 0.5 in[1] + 0.3
#          out[11] = in[1]              (head 1, channel 0)             out[11] = -in[0] + 0.1
#   (all other weights / biases zero, so every other channel of x_l + x_r is exactly 0 and contributes att*lrelu(0) = 0)
#   att[head 0] = (2, 0, ..), att[head 1] = (-1, 0, ..); output bias[0] = 0.05, bias[11] = -0.07, bias[5] = 0.5
#   edges (source -> target): 0 -> 1, 2 -> 1, 0 -> 2; self loops are added by the layer.
#
#   x_l (h0, h1): n0 (1, 2)  n1 (-1, 0.5)  n2 (0.5, -1.5)        x_r (h0, h1): n0 (1.3, -0.9)  n1 (0.55, 1.1)  n2 (-0.45, -0.4)
#   target 0, sources {0}:            alpha = 1                                   -> out = (1 + 0.05, 2 - 0.07)
#   target 1, sources {0, 2, 1}: h0:  s = (1.55, 1.05, -0.45) -> e = 2 lrelu(s) = (3.1, 2.1, -0.18)
#                                     alpha = (0.711486676, 0.261741321, 0.026772003)
#                                     out = 0.711486676*1 + 0.261741321*0.5 + 0.026772003*(-1) + 0.05 = 0.865585333
#                                h1:  s = (3.1, -0.4, 1.6) -> e = -lrelu(s) = (-3.1, 0.08, -1.6)
#                                     alpha = (0.033865653, 0.814359019, 0.151775328)
#                                     out = 0.033865653*2 + 0.814359019*(-1.5) + 0.151775328*0.5 - 0.07 = -1.147919557
#   target 2, sources {0, 2}:    h0:  s = (0.55, 0.05) -> e = (1.1, 0.1); alpha = (0.731058579, 0.268941421)
#                                     out = 0.731058579*1 + 0.268941421*0.5 + 0.05 = 0.915529289
#                                h1:  s = (1.6, -1.9) -> e = (-1.6, 0.38); alpha = (0.121318838, 0.878681162)
#                                     out = 0.121318838*2 + 0.878681162*(-1.5) - 0.07 = -1.145384067
GAT_KAT_X = ((1.0, 2.0), (-1.0, 0.5), (0.5, -1.5))                     # features 0, 1 of nodes 0..2 (features 2..21 = 0)
GAT_KAT_EDGES = ((0, 2, 0), (1, 1, 2))                                 # edge_index: row 0 = sources, row 1 = targets
GAT_KAT_OUT = {                                                       # (node, channel) -> value; every other channel = its bias
    (0, 0): 1.05, (0, 11): 1.93,
    (1, 0): 0.8655853329, (1, 11): -1.1479195571,
    (2, 0): 0.9155292893, (2, 11): -1.1453840674,
}
GAT_KAT_BIAS = {0: 0.05, 11: -0.07, 5: 0.5}
# what the two plausible misreadings would produce at (node 1, channel 0): the test asserts we are NOT there
GAT_KAT_WRONG_DIRECTION_1_0 = -0.95
GAT_KAT_WRONG_ROLES_1_0 = 0.8507363001


def gat_kat_tensors():
    """(x (3, 22), edge_index (2, 3) int64, GATv2 parameter dict keyed like the oracle's, expected (3, 22))."""
    x = torch.zeros(3, 22)
    for n, (a, b) in enumerate(GAT_KAT_X):
        x[n, 0], x[n, 1] = a, b
    Wl, Wr = torch.zeros(22, 22), torch.zeros(22, 22)
    bl, br = torch.zeros(22), torch.zeros(22)
    Wl[0, 0], Wl[11, 1] = 1.0, 1.0
    Wr[0, 1], br[0] = 0.5, 0.3
    Wr[11, 0], br[11] = -1.0, 0.1
    att = torch.zeros(1, 2, 11)
    att[0, 0, 0], att[0, 1, 0] = 2.0, -1.0
    bias = torch.zeros(22)
    for c, v in GAT_KAT_BIAS.items():
        bias[c] = v
    p = {R.P_GAT + "lin_l.weight": Wl, R.P_GAT + "lin_l.bias": bl, R.P_GAT + "lin_r.weight": Wr,
         R.P_GAT + "lin_r.bias": br, R.P_GAT + "att": att, R.P_GAT + "bias": bias}
    want = bias.view(1, 22).repeat(3, 1)
    for (n, c), v in GAT_KAT_OUT.items():
        want[n, c] = v
    return x, torch.tensor(GAT_KAT_EDGES, dtype=torch.int64), p, want
