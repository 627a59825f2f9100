"""Every GEMM epilogue combination on every kernel family against the fp64 statement of the contract
(tests/gemm_epilogue_ref.py; case table, inputs and bars: tests/gemm_epilogue_cases.py).

One test per family loops over the combinations of {row bias, pre-activation, GELU' source, residual, accumulate,
window scatter of C, split-K}, each bare (alpha only) and loaded (alpha, bias, tanh-GELU, dropout with a non-zero device
seed word), the bf16 C / bf16 pre-activation variants on tecm_gemm_bf16, and the erf-GELU set.  Every case asserts the
kernel the dispatcher picked (tecm_gemm_last_kernel), compares C -- pad columns and unmapped window rows included --
and the stored pre-activation with the reference, or asserts TecmError where the contract refuses the combination.
Failing combinations are collected and reported together.

Largest parity.elem_err seen per family on an MI355X (bar: < 1), printed again by every run with -s: the fp32 kernels
and bf16x6 0.8e-3 .. 1.3e-3, the bf16 matrix-core families on their bf16-rounded operands 0.6e-3 .. 0.8e-3 (natural
orientation, K = 4096: 2.2e-3), bf16x3 7.2e-2.  With fp32 operands and K = 40 the register-staged bf16 kernel gets one
K-tile, so split_k = 3 launches one split there and its reducer is reached through the bf16-operand family instead."""
import pytest
import torch

from tests import gemm_epilogue_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


class _Device:
    """The family's inputs on the device, in the storage the family's layouts ask for."""

    def __init__(self, inp, dev):
        fam = inp.fam
        odt = torch.bfloat16 if fam.op16 else torch.float32
        if fam.km:                                                        # A stored [k][m] with lda >= M
            self.lda = fam.lda or fam.M
            a = torch.zeros(fam.K, self.lda)
            a[:, :fam.M] = inp.A.t()
        else:
            self.lda, a = fam.K, inp.A
        self.ldb, b = (fam.N, inp.B.t().contiguous()) if fam.kn else (fam.K, inp.B)
        self.A, self.B = a.to(odt).to(dev), b.to(odt).to(dev)
        self.bias, self.rb_table = inp.bias.to(dev), inp.rb_table.to(dev)
        self.residual, self.dact, self.dact16 = inp.residual.to(dev), inp.dact.to(dev), inp.dact16.to(dev)


def _launch(ops, fam, inp, d, c, split_k, dev):
    """One ops.gemm call for the combination; returns (C buffer, its pre-fill, pre-activation buffer or None, kernel name)."""
    prefill = inp.prefill(c)
    C = prefill.to(dev)
    kw = dict(alpha=T.ALPHA, act=c.act, accumulate=c.acc, split_k=split_k if c.split else 1, bf16=fam.prec,
              a_layout=ops.A_KM if fam.km else ops.A_MK, b_layout=ops.B_KN if fam.kn else ops.B_NK)
    pre = None
    if c.bias:
        kw["bias"] = d.bias
    if c.rb:
        kw["rowbias"] = (d.rb_table, inp.ld) + inp.rowbias_spec
    if c.pre:
        pre = torch.full((fam.M, inp.ld), float("nan"), device=dev, dtype=torch.bfloat16 if c.p16 else torch.float32)
        kw["preact"] = (pre, inp.ld)
    if c.dact:
        kw["dact_src"] = (d.dact16 if c.p16 else d.dact, inp.ld)
    if c.drop:
        kw["out_drop"] = ops.drop(T.DROP_P, T.DROP_SEED, inp.drop_ld_win if c.cwin else inp.drop_ld)
    if c.res:
        kw["residual"] = (d.residual, inp.ld)
    if c.cwin:
        kw["c_win"] = ops.win(*inp.c_win)
    rec = ops.enable_gemm_timing()
    try:
        ops.gemm(fam.M, fam.N, fam.K, d.A, d.lda, d.B, d.ldb, C, inp.ldc_of(c), **kw)
        name = rec[-1][0]
    finally:
        ops.disable_gemm_timing()
    return C, prefill, pre, name


@pytest.mark.parametrize("name", [f.name for f in T.FAMILIES])
def test_every_epilogue_combination_matches_the_fp64_contract(dev, name, monkeypatch):
    from tecmollm import ops, _lib
    fam = T.FAMILY[name]
    for var in T.ENV_SWITCHES:
        monkeypatch.delenv(var, raising=False)
    for var, val in fam.env.items():
        monkeypatch.setenv(var, val)
    split_k = fam.split if fam.split > 0 else _lib.lib().tecm_gemm_tn_splits(fam.M, fam.N, fam.K)
    assert split_k >= 2
    inp = T.Inputs(fam)
    d = _Device(inp, dev)
    cases = T.enumerate_cases(fam)
    failures, compared, refused, worst, kernels = [], 0, 0, 0.0, set()
    monkeypatch.setattr(ops, "SEED_WORD", torch.tensor([T.SEED_WORD], device=dev, dtype=torch.int64))
    for c in cases:
        cname = T.case_name(c)
        if T.refusal(c):                                                  # refused by contract: nothing may be launched
            refused += 1
            try:
                _launch(ops, fam, inp, d, c, split_k, dev)
                failures.append(f"{cname}: not refused")
            except _lib.TecmError:
                pass
            continue
        compared += 1
        try:
            C, prefill, pre, kernel = _launch(ops, fam, inp, d, c, split_k, dev)
        except _lib.TecmError as e:
            failures.append(f"{cname}: refused ({e})")
            continue
        kernels.add(kernel)
        if kernel != T.expected_kernel(fam, c):
            failures.append(f"{cname}: ran {kernel}, expected {T.expected_kernel(fam, c)}")
        fails, err = T.check_case(inp, c, C, pre, prefill)
        worst = max(worst, err or 0.0)
        failures += [f"{cname}: {f}" for f in fails]
    print(f"\n{name}: {compared} compared, {refused} refused, largest elem_err {worst:.3g}, kernels {sorted(kernels)}")
    assert compared + refused == len(cases) and refused == len(T.refused_list(fam))
    assert not failures, f"{len(failures)} failing: " + "; ".join(failures)
