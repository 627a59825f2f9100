"""CPU tests that keep the fp64 statement of the GEMM epilogue contract (tests/gemm_epilogue_ref.py) honest: against
torch's own ops on compositions the model uses, and -- for every combination the GPU matrix enumerates -- that the same
epilogue evaluated in fp32 meets the bars the kernels are held to (tests/gemm_epilogue_cases.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_epilogue_cases as T
from tests import gemm_epilogue_ref as R


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64)


def test_linear_tanh_gelu_with_preactivation():
    M, N, K = 37, 20, 16
    x, w, b = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=0.3), _rand(N, seed=3)
    out, pre, _ = R.epilogue_ref(x @ w.t(), _nan(M, N + 3), N + 3, bias=b, act=R.ACT_GELU_TANH,
                                 preact=(torch.empty(0), N))
    lin = F.linear(x, w, b)
    torch.testing.assert_close(pre, lin, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(out[:, :N], F.gelu(lin, approximate="tanh"), rtol=1e-12, atol=1e-13)
    assert bool(torch.isnan(out[:, N:]).all())


@pytest.mark.parametrize("act,approx", [(R.ACT_GELU_ERF, "none"), (R.ACT_GELU_TANH, "tanh")])
def test_gelu_and_its_autograd_derivative(act, approx):
    M, N = 29, 24
    P, src = _rand(M, N, seed=4), _rand(M, N, seed=5, scale=2.0)
    out, _, _ = R.epilogue_ref(P, _nan(M, N), N, act=act)
    torch.testing.assert_close(out, F.gelu(P, approximate=approx), rtol=1e-12, atol=1e-13)
    s = src.clone().requires_grad_(True)
    (grad,) = torch.autograd.grad(F.gelu(s, approximate=approx).sum(), s)
    out, _, _ = R.epilogue_ref(P, _nan(M, N), N, act=act, dact_src=(src, N))
    torch.testing.assert_close(out, P * grad, rtol=1e-11, atol=1e-12)          # the derivative REPLACES the activation
    with pytest.raises(ValueError):
        R.epilogue_ref(P, _nan(M, N), N, act=R.ACT_NONE, dact_src=(src, N))


def test_dropout_with_an_explicit_mask_then_residual_then_previous_c():
    from tecmollm.rng import keep_mult
    M, N, ld, p, seed, word = 50, 40, 47, 0.1, 0xABCDEF0123456789, 5
    P, res, prev = _rand(M, N, seed=6), _rand(M, N, seed=7), _rand(M, N, seed=8)
    out, _, mult = R.epilogue_ref(P, prev, N, alpha=0.5, out_drop=(p, seed, ld), seed_word=word, residual=(res, N),
                                  accumulate=True)
    idx = (np.arange(M)[:, None] * ld + np.arange(N)[None, :]).astype(np.uint64)
    mask = torch.from_numpy(keep_mult(seed + word, idx, p)).double()
    assert 0.05 < float((mask == 0).double().mean()) < 0.15 and torch.equal(mask, mult.double())
    assert not torch.equal(mask, torch.from_numpy(keep_mult(seed, idx, p)).double())     # the word moves the masks
    torch.testing.assert_close(out, (0.5 * P) * mask + res + prev, rtol=1e-13, atol=1e-13)


def test_window_scatter_is_the_transpose_of_the_patch_rearrangement():
    """'b (p l) d -> b p (l d)' of modules.py:114 backwards, as test_gemm_window_stride2_and_patch_and_cwin builds it, with a
    tail time step no row maps to and an out-of-range tap that must be dropped."""
    Bn, P, nodes, pl, D = 2, 3, 5, 4, 6
    Lin = P * pl + 1
    Pm = _rand(Bn * P * nodes, pl * D, seed=9)
    out, _, _ = R.epilogue_ref(Pm, _nan(Bn * Lin * nodes, D + 2), D + 2, c_win=(nodes, Lin, P, pl, pl, D, 0))
    out = out.view(Bn, Lin, nodes, D + 2)
    want = Pm.view(Bn, P, nodes, pl, D).permute(0, 1, 3, 2, 4).reshape(Bn, P * pl, nodes, D)
    assert torch.equal(out[:, :P * pl, :, :D], want)
    assert bool(torch.isnan(out[:, P * pl:]).all()) and bool(torch.isnan(out[..., D:]).all())
    # pad = 1: tap 0 of the first step falls on t_in = -1 and is dropped; mask indices are those of the TARGET element
    out, _, mult = R.epilogue_ref(Pm, _nan(Bn * Lin * nodes, D), D, c_win=(nodes, Lin, P, pl, pl, D, 1),
                                  out_drop=(0.5, 11, D + 1))
    out = out.view(Bn, Lin, nodes, D)
    from tecmollm.rng import keep_mult
    rows = (np.arange(Bn * Lin * nodes)[:, None] * (D + 1) + np.arange(D)[None, :]).astype(np.uint64)
    mask = torch.from_numpy(keep_mult(11, rows, 0.5)).double().view(Bn, Lin, nodes, D)
    src = Pm.view(Bn, P, nodes, pl, D).permute(0, 1, 3, 2, 4).reshape(Bn, P * pl, nodes, D)
    assert torch.equal(out[:, :P * pl - 1], src[:, 1:] * mask[:, :P * pl - 1])
    assert bool(torch.isnan(out[:, P * pl - 1:]).all())


def test_bf16_preactivation_is_rounded_before_the_activation():
    M, N = 33, 16
    P = _rand(M, N, seed=12)
    out, pre, _ = R.epilogue_ref(P, _nan(M, N), N, act=R.ACT_GELU_TANH, preact=(torch.empty(0, dtype=torch.bfloat16), N))
    assert torch.equal(pre, P.float().bfloat16().double())
    torch.testing.assert_close(out, F.gelu(pre, approximate="tanh"), rtol=1e-12, atol=1e-13)


def test_every_family_enumerates_and_refuses_what_the_contract_says():
    for fam in T.FAMILIES:
        cases = T.enumerate_cases(fam)
        refused = T.refused_list(fam)
        assert len(cases) == (2 * 128 + 64 + 4 if fam.prec != 1 else 2 * 128 * 2 + 2 * 96 * 2 + 64 + 6), fam.name
        assert "bare+dact+actnone" in refused and "erf+cwin" in refused and "erf+res" in refused and "erf+acc" in refused
        if fam.prec == 1:
            for name in ("bare+res+c16", "bare+pre+split+p16", "erf+c16", "erf+pre+p16", "loaded+cwin+c16", "bare+rb+pre+p16"):
                assert name in refused, (fam.name, name)
        else:
            assert len(refused) == 4
        for c in cases:
            T.expected_kernel(fam, c)                               # every combination has an expected kernel


def _classes():
    """Families that differ only in the kernel share their inputs' arithmetic: one representative per (shape, operand
    rounding, set of variants)."""
    seen, out = set(), []
    for fam in T.FAMILIES:
        key = (fam.M, fam.N, fam.K, fam.prec == 1)
        if key not in seen:
            seen.add(key)
            out.append(fam.name)
    return out


@pytest.mark.parametrize("name", _classes())
def test_fp32_arithmetic_meets_the_bars_of_the_gpu_matrix(name):
    """The epilogue of every enumerated, accepted combination evaluated in fp32 on the CPU (product included) passes the
    comparison the GPU kernels are held to: the bars leave room for correct fp32 arithmetic."""
    fam = T.FAMILY[name]
    inp = T.Inputs(fam)
    P32 = inp.A @ inp.B.t()
    failures, compared, refused, worst = [], 0, 0, 0.0
    for c in T.enumerate_cases(fam):
        if T.refusal(c):
            refused += 1
            continue
        prefill = inp.prefill(c)
        got, pre, _ = R.epilogue_ref(P32, prefill.float(), inp.ldc_of(c), dtype=torch.float32, **inp.ref_kwargs(c))
        got_pre = None
        if c.pre:
            got_pre = torch.full((fam.M, inp.ld), float("nan"))
            got_pre[:, :fam.N] = pre
            if c.p16:
                got_pre = got_pre.bfloat16()
        fails, err = T.check_case(inp, c, got.bfloat16() if c.c16 else got, got_pre, prefill)
        compared += 1
        worst = max(worst, err or 0.0)
        failures += [f"{T.case_name(c)}: {f}" for f in fails]
    assert not failures, failures
    assert compared + refused == len(T.enumerate_cases(fam)) and compared > 0
    assert worst < 0.1                                               # fp32 rounding sits far inside the element bar
