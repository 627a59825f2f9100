"""Query 0 of a causal sequence sees one key, so its softmax is 1 and its score gradient 0 whatever q_0 is.  The fp32 step uses
that three ways, and each is held to "bit for bit what the full computation gives":

  1  TecmGemm's dead-rectangle hint: block tiles whose whole output lies in (row % period < rows, col < cols) are not computed
     and nothing is stored for them (the c_attn forward: the q columns of the token-0 rows);
  2  TecmGemm's zero-rectangle hint: block tiles whose rows of A are known zeros for k < zero_k start their K loop there (the
     d c_attn launches: dq_0 = 0);
  3  the compile-time-T attention kernels load no q_0, give its row p = 1 and write dq_0 = +0;
  4  GPT2StackFn with TECM_CAUSAL_Q0=1 (default) against =0: the output and every gradient.

Shapes: M = 2 * 3 * 300 rows, i.e. two sequences' worth of T = 3 tokens over N = 300 nodes -- the token-0 runs start at row 0
(tile aligned) and at row 900 = 7 * 128 + 4 (not aligned), and M is no multiple of the 128-row tile.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_cpu as R  # noqa: E402

pytestmark = pytest.mark.gpu

NODES, T3 = 300, 3
M = 2 * T3 * NODES            # 1800
PERIOD = T3 * NODES           # 900
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _rand(*shape, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dev)


def _dead_tiles(Mr, Nc, bm, bn, period, rows, cols):
    """Brute force, element by element: boolean (tiles_m, tiles_n) map of the tiles wholly inside the rectangle."""
    r, c = np.arange(Mr), np.arange(Nc)
    inside = ((r % period) < rows)[:, None] & (c < cols)[None, :]
    tm, tn = -(-Mr // bm), -(-Nc // bn)
    return np.array([[inside[i * bm:(i + 1) * bm, j * bn:(j + 1) * bn].all() for j in range(tn)] for i in range(tm)])


def _tile_mask(tiles, Mr, Nc, bm, bn, dev):
    m = np.kron(tiles.astype(np.uint8), np.ones((bm, bn), dtype=np.uint8))[:Mr, :Nc].astype(bool)
    return torch.from_numpy(m).to(dev)


# ------------------------------------------------------------------------------------------------ 1: dead rectangle
@pytest.fixture(scope="module")
def dead_case(dev):
    from tecmollm import ops
    N, K = 768, 288
    A, B, bias = _rand(M, K, dev=dev, seed=1), 0.1 * _rand(N, K, dev=dev, seed=2), _rand(N, dev=dev, seed=3)
    ref = torch.full((M, N), NAN, device=dev)
    ops.gemm(M, N, K, A, K, B, K, ref, N, bias=bias)
    assert bool(torch.isfinite(ref).all())
    return N, K, A, B, bias, ref


def _run_dead(dead_case, rect, dev):
    from tecmollm import ops
    N, K, A, B, bias, _ = dead_case
    out = torch.full((M, N), NAN, device=dev)
    ops.gemm(M, N, K, A, K, B, K, out, N, bias=bias, dead_rect=rect)
    return out, int(ops.lib().tecm_gemm_last_skipped_flops())


def test_dead_rectangle_skips_whole_tiles_and_stores_nothing_there(dev, dead_case):
    from tecmollm import ops
    N, K, _, _, _, ref = dead_case
    out, skipped = _run_dead(dead_case, (PERIOD, NODES, 256), dev)
    tiles = _dead_tiles(M, N, 128, 128, PERIOD, NODES, 256)
    # row tiles 0, 1 (run at row 0) and 8 (run at row 900: tile 7 holds rows 896..899 of the previous token) x 2 column tiles
    assert sorted(zip(*np.nonzero(tiles))) == [(0, 0), (0, 1), (1, 0), (1, 1), (8, 0), (8, 1)]
    mask = _tile_mask(tiles, M, N, 128, 128, dev)
    assert torch.equal(out[~mask], ref[~mask])
    assert bool(torch.isnan(out[mask]).all())
    untouched = sum(bool(torch.isnan(out[i * 128:(i + 1) * 128, j * 128:(j + 1) * 128]).all())      # still all NaN
                    for i in range(-(-M // 128)) for j in range(N // 128))
    assert untouched == int(tiles.sum()) == ops.lib().tecm_gemm_rect_tiles(M, N, 128, 128, PERIOD, NODES, 256) == 6
    assert int(torch.isnan(out).sum()) == 6 * 128 * 128
    assert skipped == 2 * 6 * 128 * 128 * K                                 # what the timing records subtract from 2 M N K


def test_a_partly_dead_column_tile_is_computed(dev, dead_case):
    from tecmollm import ops
    N, K, _, _, _, ref = dead_case
    out, skipped = _run_dead(dead_case, (PERIOD, NODES, 200), dev)
    tiles = _dead_tiles(M, N, 128, 128, PERIOD, NODES, 200)
    assert int(tiles.sum()) == 3 == ops.lib().tecm_gemm_rect_tiles(M, N, 128, 128, PERIOD, NODES, 200) and not tiles[:, 1:].any()
    mask = _tile_mask(tiles, M, N, 128, 128, dev)
    assert torch.equal(out[~mask], ref[~mask]) and bool(torch.isnan(out[mask]).all())
    assert torch.equal(out[:, 128:256], ref[:, 128:256])                     # columns 128..199 are "dead", their tile is not
    assert skipped == 2 * 3 * 128 * 128 * K


def test_no_tile_fits_a_hundred_dead_rows(dev, dead_case):
    from tecmollm import ops
    N, _, _, _, _, ref = dead_case
    out, skipped = _run_dead(dead_case, (PERIOD, 100, 256), dev)
    assert ops.lib().tecm_gemm_rect_tiles(M, N, 128, 128, PERIOD, 100, 256) == 0 and skipped == 0
    assert torch.equal(out, ref)


def test_dead_rectangle_is_ignored_where_another_pass_walks_all_of_c(dev, dead_case):
    """split_k > 1: the reducer writes every element of C from the workspace, so no tile may be left out."""
    from tecmollm import ops
    N, K, A, B, bias, _ = dead_case
    ref, out = torch.full((M, N), NAN, device=dev), torch.full((M, N), NAN, device=dev)
    ops.gemm(M, N, K, A, K, B, K, ref, N, bias=bias, split_k=2)
    ops.gemm(M, N, K, A, K, B, K, out, N, bias=bias, split_k=2, dead_rect=(PERIOD, NODES, 256))
    assert int(ops.lib().tecm_gemm_last_skipped_flops()) == 0
    assert torch.equal(out, ref)


# ------------------------------------------------------------------------------------------------ 2: zero rectangle
K2, ZK = 768, 256
FULL_ROWS = [(0, 256), (1024, 1152)]           # the rows of row tiles 0, 1 and 8: the tiles wholly inside the rectangle


def _zero_a(dev, zero):
    A = _rand(M, K2, dev=dev, seed=5)
    rows = (torch.arange(M, device=dev) % PERIOD) < NODES
    A[rows, :ZK] = zero
    return A


@pytest.mark.parametrize("zero", [0.0, -0.0], ids=["+0", "-0"])
@pytest.mark.parametrize("N", [256, 32], ids=["tile128", "tile32"])
def test_zero_rectangle_gives_the_full_loops_bits_and_does_not_read_the_range(dev, N, zero):
    from tecmollm import ops
    A = _zero_a(dev, zero)
    assert bool((torch.signbit(A[0, :ZK]) == (str(zero) == "-0.0")).all())
    B, bias = 0.1 * _rand(N, K2, dev=dev, seed=6), _rand(N, dev=dev, seed=7)
    rect = (PERIOD, NODES, ZK)
    ref, out, out_nan = (torch.full((M, N), NAN, device=dev) for _ in range(3))
    ops.gemm(M, N, K2, A, K2, B, K2, ref, N, bias=bias)
    assert ops.lib().tecm_gemm_last_kernel().decode() == f"gemm_kernel<0,0,4,4,{128 if N > 64 else 32},false,false,128>"
    ops.gemm(M, N, K2, A, K2, B, K2, out, N, bias=bias, zero_rect=rect)
    assert int(ops.lib().tecm_gemm_last_skipped_flops()) == 2 * 3 * 128 * N * ZK
    assert torch.equal(out, ref)
    for r0, r1 in FULL_ROWS:                           # NaN where only whole tiles look: a read of the range would show
        A[r0:r1, :ZK] = NAN
    ops.gemm(M, N, K2, A, K2, B, K2, out_nan, N, bias=bias, zero_rect=rect)
    assert torch.equal(out_nan, ref)


def test_zero_rectangle_is_ignored_under_split_k_a_window_or_dropout(dev):
    from tecmollm import ops
    N = 256
    A = _zero_a(dev, 0.0)
    B = 0.1 * _rand(N, K2, dev=dev, seed=6)
    rect = (PERIOD, NODES, ZK)
    # a window view of a (1, 6, 300, 256) tensor: 3 taps of 256 channels, pad 1 -> M = 1800 rows of K = 768
    src = _rand(6 * NODES, 256, dev=dev, seed=8)
    w = ops.win(NODES, 6, 6, 1, 3, 256, 1)
    variants = {"split_k": dict(A=A, lda=K2, kw=dict(split_k=2)),
                "dropout": dict(A=A, lda=K2, kw=dict(a_drop=ops.drop(0.1, 99, K2))),
                "window": dict(A=src, lda=256, kw=dict(a_win=w))}
    for name, v in variants.items():
        ref, out = torch.full((M, N), NAN, device=dev), torch.full((M, N), NAN, device=dev)
        ops.gemm(M, N, K2, v["A"], v["lda"], B, K2, ref, N, **v["kw"])
        ops.gemm(M, N, K2, v["A"], v["lda"], B, K2, out, N, zero_rect=rect, **v["kw"])
        assert int(ops.lib().tecm_gemm_last_skipped_flops()) == 0, name
        assert bool(torch.isfinite(ref).all()) and torch.equal(out, ref), name


# ------------------------------------------------------------------------------------------------ 3: attention
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop"])
@pytest.mark.parametrize("q16", [False, True], ids=["fp32", "bf16qkv"])
@pytest.mark.parametrize("T", [3, 6, 8, 12])
def test_attention_does_not_touch_q0(dev, T, q16, p):
    from tecmollm import ops
    assert not ops.attention_reads_q0(T)
    B, N, H, D = 2, 37, 12, 768
    rows = B * T * N
    qkv = _rand(rows, 3 * D, dev=dev, seed=10 + T)
    dctx = _rand(rows, D, dev=dev, seed=20 + T)
    if q16:
        qkv = qkv.to(torch.bfloat16)
    tok0 = (torch.arange(rows, device=dev) // N) % T == 0
    qkv_nan = qkv.clone()
    qkv_nan[tok0, :D] = NAN
    spec = ops.drop(p, 4242, 1) if p > 0 else None
    res = []
    for x in (qkv, qkv_nan):
        ctx = torch.full((rows, D), NAN, device=dev)
        dqkv = torch.full((rows, 3 * D), NAN, device=dev)
        ops.attention_fwd(x, ctx, B, T, N, H, D, spec)
        ops.attention_bwd(x, dctx, dqkv, B, T, N, H, D, spec)
        assert bool((dqkv[tok0, :D] == 0).all())                             # dq_0, exactly
        res.append((ctx, dqkv))
    assert bool(torch.isfinite(res[0][0]).all()) and bool(torch.isfinite(res[0][1]).all())
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    if p > 0:                                                                # the mask reaches row 0 too: p = 1 * keep / (1 - p)
        v0 = qkv[tok0, 2 * D:].float()
        ratio = res[0][0][tok0] / v0
        assert bool(((ratio == 0) | ((ratio - 1 / 0.9).abs() < 1e-6)).all()) and bool((ratio == 0).any())


def test_the_library_says_which_t_read_q0(dev):
    from tecmollm import ops
    assert [t for t in range(1, 40) if not ops.attention_reads_q0(t)] == [1, 2, 3, 4, 6, 8, 12]
    assert ops.attention_reads_q0(21) and ops.attention_reads_q0(45)


# ------------------------------------------------------------------------------------------------ 4: the stack
@pytest.fixture(scope="module")
def backbone(dev):
    from src.model.modules import LLMBackbone
    cfg = R.default_config(L_in=48, num_nodes=NODES, llm_layers=3)
    p = R.init_params(cfg, seed=45)
    bb = LLMBackbone(3, include_wte=False, load_pretrained=False)
    bb.load_state_dict({k[len("llm_backbone."):]: v for k, v in p.items() if k.startswith("llm_backbone.")})
    return bb.to(dev).train()


@pytest.mark.parametrize("T", [3, 6])
def test_stack_with_the_hints_equals_the_stack_without(dev, backbone, T, monkeypatch):
    """B = 2, N = 300, three layers, training mode (p = 0.1, pinned seeds): output, d input and every parameter gradient."""
    from tecmollm import functions as F_
    B, D = 2, 768
    h0 = (0.5 * _rand(B, T, NODES, D, dev=dev, seed=30 + T)).requires_grad_(True)
    gout = _rand(B, T, NODES, D, dev=dev, seed=40 + T)
    params = [q for q in backbone.parameters() if q.requires_grad and q.dim() > 0]
    seen = []
    real_gemm = F_.gemm

    def spy(*a, **k):
        seen.append((k.get("dead_rect"), k.get("zero_rect")))
        return real_gemm(*a, **k)
    monkeypatch.setattr(F_, "gemm", spy)
    runs = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("TECM_CAUSAL_Q0", switch)
        seen.clear()
        out = backbone.forward_tm(h0, F_.DropPlan(True, 0.1, 4711))
        grads = torch.autograd.grad(out, [h0] + params, gout, allow_unused=True)
        runs[switch] = (out.detach().clone(), grads, list(seen))
    rect = (T * NODES, NODES, D)
    assert all(d is None and z is None for d, z in runs["0"][2])
    assert [d for d, _ in runs["1"][2]].count(rect) == 3 and [z for _, z in runs["1"][2]].count(rect) == 6
    assert bool(torch.isfinite(runs["1"][0]).all())
    assert torch.equal(runs["0"][0], runs["1"][0])
    used = 0
    for a, b in zip(runs["0"][1], runs["1"][1]):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)
            used += 1
    assert used >= 1 + 3 * 6 + 2                       # d h0; per layer ln_1, ln_2 (w, b), lora_A, lora_B; ln_f
