"""Case table of the GEMM epilogue matrix (tests/test_gpu_gemm_epilogue.py, tests/test_host_gemm_epilogue_ref.py): the
kernel families with the kernel the dispatcher must pick for every combination, the combinations, the ones the entry
point refuses by contract, the inputs, and the comparison against tests/gemm_epilogue_ref.py under the project's bars."""
import itertools
from collections import namedtuple

import torch

from tests import gemm_epilogue_ref as R
from tests.parity import elem_err

ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH = R.ACT_NONE, R.ACT_GELU_ERF, R.ACT_GELU_TANH
ENV_SWITCHES = ("TECM_BF16_DMA", "TECM_BF16_P8", "TECM_BF16_TN", "TECM_BF16_TALL", "TECM_P8_ROWS")

# ------------------------------------------------------------------------------------------------ families
# prec: the precision code of ops.gemm (0 exact fp32, 1 bf16 matrix cores, 2 bf16x3, 3 bf16x6); op16: A and B are bf16
# tensors; km / kn: A stored [k][m] / B stored [k][n]; lda: leading dimension of A where it is not the natural one;
# batch = (B, P, nodes) with M = B * P * nodes: the rows as the row bias and the window view of C read them;
# split: the split_k asked for when the combination splits K (-1: what tecm_gemm_tn_splits returns for the shape).
Family = namedtuple("Family", "name M N K prec op16 km kn lda batch env split")


def factor_rows(M):
    """M = B * P * nodes: B the smallest prime factor of M, P the smallest prime factor of what is left, nodes the rest
    (258 -> (2, 3, 43), 64 -> (2, 2, 16); a prime M -> (M, 1, 1))."""
    def spf(n):
        return next((d for d in range(2, int(n ** 0.5) + 1) if n % d == 0), n)
    b = spf(M)
    p = spf(M // b)
    return b, p, M // (b * p)


def _fam(name, M, N, K, prec=0, op16=False, km=False, kn=False, lda=None, env=None, split=3, batch=None):
    batch = tuple(batch) if batch else factor_rows(M)
    assert batch[0] * batch[1] * batch[2] == M
    return Family(name, M, N, K, prec, op16, km, kn, lda, batch, dict(env or {}), split)


FAMILIES = [
    _fam("f32_mk_nk_vec4", 258, 264, 36),
    _fam("f32_mk_nk_scalar", 258, 262, 36),                         # N % 4 != 0: the scalar epilogue
    _fam("f32_general", 258, 264, 37),                              # K % 2 != 0: the general instance
    _fam("f32_mk_kn", 258, 264, 36, kn=True),
    _fam("f32_km_kn", 258, 264, 36, km=True, kn=True, lda=260),     # lda % 4 == 0: the float4 loaders, 128-row tile
    _fam("f32_km_kn_m64", 64, 264, 36, km=True, kn=True),           # M <= 64: the 64-row tile
    _fam("bf16_reg_f32ops", 258, 264, 40, prec=1),
    _fam("bf16_reg_op16", 258, 264, 128, prec=1, op16=True, env={"TECM_BF16_DMA": "0"}),
    _fam("bf16_dma", 258, 264, 128, prec=1, op16=True, env={"TECM_BF16_DMA": "1"}),
    _fam("bf16_dma2", 258, 264, 128, prec=1, op16=True, env={"TECM_BF16_DMA": "2"}),
    _fam("bf16_dma5", 258, 264, 128, prec=1, op16=True, env={"TECM_BF16_DMA": "5"}),
    _fam("bf16_p8_128", 258, 264, 128, prec=1, op16=True, env={"TECM_BF16_P8": "1", "TECM_P8_ROWS": "128"}),
    _fam("bf16_p8_112", 258, 264, 128, prec=1, op16=True, env={"TECM_BF16_P8": "1", "TECM_P8_ROWS": "112"}),
    _fam("bf16_p8_96", 258, 264, 128, prec=1, op16=True, env={"TECM_BF16_P8": "1", "TECM_P8_ROWS": "96"}),
    _fam("bf16_tn", 64, 192, 4096, prec=1, op16=True, km=True, kn=True, split=-1),
    _fam("bf16x3", 258, 264, 36, prec=2),
    _fam("bf16x6", 258, 264, 36, prec=3),
]
FAMILY = {f.name: f for f in FAMILIES}

# ------------------------------------------------------------------------------------------------ combinations
Case = namedtuple("Case", "load rb pre dact res acc cwin split bias act drop c16 p16")


def case_name(c):
    parts = [c.load]
    parts += [k for k, on in (("bias", c.bias and c.load == "erf"), ("rb", c.rb), ("pre", c.pre), ("dact", c.dact),
                              ("drop", c.drop and c.load == "erf"), ("res", c.res), ("acc", c.acc), ("cwin", c.cwin),
                              ("split", c.split), ("c16", c.c16), ("p16", c.p16)) if on]
    if c.dact and c.act == ACT_NONE:
        parts.append("actnone")
    return "+".join(parts)


def enumerate_cases(fam):
    """Every combination of the switches that decide the epilogue path, bare and loaded; for tecm_gemm_bf16 the bf16 C and
    bf16 pre-activation variants of each; the erf-GELU set; and the combinations named in the contract as refused."""
    cases = []
    for rb, pre, dact, res, acc, cwin, split in itertools.product((False, True), repeat=7):
        for load in ("bare", "loaded"):
            loaded = load == "loaded"
            base = Case(load, rb, pre, dact, res, acc, cwin, split, bias=loaded,
                        act=ACT_GELU_TANH if (loaded or dact) else ACT_NONE, drop=loaded, c16=False, p16=False)
            cases.append(base)
            if fam.prec == 1:
                cases.append(base._replace(c16=True))
                if pre or dact:                                   # a bf16 pre-activation exists only where one is passed
                    cases.append(base._replace(p16=True))
                    cases.append(base._replace(c16=True, p16=True))
    for dact in (False, True):
        for bias, rb, pre, drop, split in itertools.product((False, True), repeat=5):
            cases.append(Case("erf", rb, pre, dact, False, False, False, split, bias, ACT_GELU_ERF, drop, False, False))
    erf = Case("erf", False, False, False, False, False, False, False, False, ACT_GELU_ERF, False, False, False)
    cases += [erf._replace(res=True), erf._replace(acc=True), erf._replace(cwin=True)]
    if fam.prec == 1:
        cases += [erf._replace(c16=True), erf._replace(pre=True, p16=True)]
    cases.append(Case("bare", False, False, True, False, False, False, False, False, ACT_NONE, False, False, False))
    assert len({case_name(c) for c in cases}) == len(cases)
    return cases


def refusal(c):
    """The reason tecm_gemm_* refuses the combination by contract (include/tecmollm.h), or None."""
    if c.dact and c.act == ACT_NONE:
        return "dact_src needs act to name the activation whose derivative is taken"
    if c.act == ACT_GELU_ERF and (c.res or c.acc or c.cwin):
        return "erf-GELU takes no residual / accumulate / c_win"
    if c.p16 and (c.split or c.cwin or c.rb or c.act == ACT_GELU_ERF):
        return "a bf16 pre-activation needs the plain tanh-GELU epilogue: no split_k / c_win / row bias / erf"
    if c.c16 and (c.res or c.acc or c.cwin or c.split or c.act == ACT_GELU_ERF):
        return "a bf16 C needs the plain epilogue: no residual / accumulate / c_win / split_k / erf"
    return None


def refused_list(fam):
    return {case_name(c): refusal(c) for c in enumerate_cases(fam) if refusal(c)}


# ------------------------------------------------------------------------------------------------ expected kernel
def expected_kernel(fam, c):
    """Name tecm_gemm_last_kernel must report, read off the dispatchers: csrc/gemm.hip (gemm_entry), gemm_{mk_nk,mk_kn,
    km_kn}.hip + gemm_impl.h (dispatch, dispatch_m64), gemm_bf16_{mk_nk,km_kn}.hip, tecm_gemm16_dma_try, tecm_gemm16_p8_try,
    tecm_gemm16_tn_try, gemm_x3.hip."""
    if fam.prec == 2:
        return "gemm_x3_kernel<2,32>"
    if fam.prec == 3:
        return "gemm_x3_kernel<3,16>"
    lay = f"{int(fam.km)},{int(fam.kn)}"
    if fam.prec == 0:
        if fam.K % 2:                                       # pick_vec: K % 2 != 0 leaves scalar loaders -> the general instance
            return f"gemm_kernel<{lay},1,1,128,true,true,128>"
        assert fam.K % 4 == 0 and (not fam.km or (fam.lda or fam.M) % 4 == 0)      # everything else: the float4 loaders
        return f"gemm_kernel<{lay},4,4,128,false,false,{64 if fam.km and fam.M <= 64 else 128}>"
    if not fam.op16:
        return f"gemm_bf16_kernel<{lay},false,false>"
    if fam.km:                                              # both operands bf16, KM x KN: natural orientation from split_k = 2 on
        return "gemm_bf16_tn_kernel" if c.split else "gemm_bf16_kernel<1,1,true,false>"
    reg = "gemm_bf16_kernel<0,0,false,false>"
    dma = fam.env.get("TECM_BF16_DMA")
    if c.split or dma == "0":
        return reg
    erf = c.act == ACT_GELU_ERF                             # erf: the GEMM runs with a plain epilogue, erf_post_kernel finishes
    streams = int(c.res) + int(c.dact and not erf) + int(c.acc)
    if c.cwin:
        fast = streams == 0 and not c.rb and not c.pre and not c.c16 and not c.p16
    else:
        fast = streams == 0 if c.rb else streams <= 1
    if dma is None:                                         # TECM_BF16_P8 = 1: eight phases wherever the straight-line epilogue serves
        if fast:
            return f"gemm_bf16_p8_kernel<{fam.env['TECM_P8_ROWS']}>"
        return "gemm_bf16_dma2_kernel"                      # N % 256 = 8: the 128-column geometry
    if dma == "2":
        return "gemm_bf16_dma2_kernel"
    if dma == "5" and not c.cwin and not c.rb and streams <= 1:
        return "gemm_bf16_dma5_kernel"
    return "gemm_bf16_dma_kernel"


# ------------------------------------------------------------------------------------------------ inputs
ALPHA = 0.5
DROP_P = 0.1
DROP_SEED = 0x5EED0123456789AB
SEED_WORD = 0x0000000300000007            # non-zero in both halves: a kernel that ignores the word draws other masks
TAPS = 2


class Inputs:
    """CPU tensors of one family, drawn once: A, B ~ N(0,1) K^(-1/4) (product O(1); rounded to bf16 where the family's
    matrix cores read bf16), everything the epilogue adds or multiplies by ~ N(0,1)."""

    def __init__(self, fam):
        # families that differ only in the kernel draw the SAME inputs: the host test's fp32 evaluation of one stands for all
        g = torch.Generator().manual_seed(20240 + 7 * fam.M + 3 * fam.N + fam.K + (1000 if fam.prec == 1 else 0))
        M, N, K = fam.M, fam.N, fam.K
        s = float(K) ** -0.25
        self.fam = fam
        self.A = self.draw_operand(g, M, K) * s
        self.B = self.draw_operand(g, N, K) * s
        if fam.prec == 1:
            self.A, self.B = R.round_bf16(self.A), R.round_bf16(self.B)
        self.P = self.A.double() @ self.B.double().t()
        Bq, Pp, nodes = fam.batch
        self.Cw = N // TAPS
        self.Lout, self.Lin = Pp, Pp * TAPS + 1            # a tail time step no row maps to
        self.c_win = (nodes, self.Lin, self.Lout, TAPS, TAPS, self.Cw, 0)
        self.win_rows = Bq * self.Lin * nodes
        pad = 4 if N % 4 == 0 else 5
        self.ldc, self.ldc_win = N + pad, self.Cw + pad
        self.ld = N + 4                                     # of the row-bias table, pre-activation, GELU' source, residual
        self.drop_ld, self.drop_ld_win = self.ldc + 3, self.ldc_win + 3       # the mask's own leading dimension
        self.bias = torch.randn(N, generator=g)
        self.rb_table = torch.randn(Pp, self.ld, generator=g)
        self.rowbias_spec = (nodes, Pp)                     # rb_div, rb_mod
        self.residual = torch.randn(M, self.ld, generator=g)
        self.dact = torch.randn(M, self.ld, generator=g)
        self.dact16 = self.dact.bfloat16()
        self.prev = torch.randn(M, self.ldc, generator=g)
        self.prev_win = torch.randn(self.win_rows, self.ldc_win, generator=g)

    @staticmethod
    def draw_operand(g, rows, K):
        """(rows, K) operand before the K^(-1/4) scale; a subclass may draw another distribution."""
        return torch.randn(rows, K, generator=g)

    def prefill(self, c):
        """C before the call: NaN, or the previous C when accumulating, always with NaN sentinels in the pad columns."""
        prev, width = (self.prev_win, self.Cw) if c.cwin else (self.prev, self.fam.N)
        buf = prev.clone() if c.acc else torch.full_like(prev, float("nan"))
        buf[:, width:] = float("nan")
        return buf.bfloat16() if c.c16 else buf

    def ref_kwargs(self, c):
        """Keyword arguments of epilogue_ref for the combination (CPU tensors)."""
        pre_dt = torch.bfloat16 if c.p16 else torch.float32
        kw = dict(alpha=ALPHA, act=c.act, accumulate=c.acc, c_bf16=c.c16)
        if c.bias:
            kw["bias"] = self.bias
        if c.rb:
            kw["rowbias"] = (self.rb_table, self.ld) + self.rowbias_spec
        if c.pre:
            kw["preact"] = (torch.empty(0, dtype=pre_dt), self.ld)
        if c.dact:
            kw["dact_src"] = (self.dact16 if c.p16 else self.dact, self.ld)
        if c.drop:
            kw["out_drop"] = (DROP_P, DROP_SEED, self.drop_ld_win if c.cwin else self.drop_ld)
            kw["seed_word"] = SEED_WORD
        if c.res:
            kw["residual"] = (self.residual, self.ld)
        if c.cwin:
            kw["c_win"] = self.c_win
        return kw

    def ldc_of(self, c):
        return self.ldc_win if c.cwin else self.ldc


# ------------------------------------------------------------------------------------------------ comparison
TOL = 2e-4                                # max-norm bar of tests/test_gpu_ops.py


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _bf16_bar(got, ref):
    """|got - ref| <= 2^-7 |ref| + 1e-6 per element (one bf16 ulp; tests/test_gpu_bf16.py): worst ratio, < = 1 passes."""
    return float(((got - ref).abs() / (ref.abs() * 2.0 ** -7 + 1e-6)).max())


_checked_masks = set()


def check_case(inp, c, got_c, got_pre, prefill):
    """Compare what a call left in C (and in the pre-activation) with the contract.  got_c / prefill: the whole buffers
    (fp32 or bf16), got_pre: the (M, ld) pre-activation buffer or None.  Returns (failure strings, elem_err or None)."""
    fam = inp.fam
    M, N = fam.M, fam.N
    kw = inp.ref_kwargs(c)
    ldc = inp.ldc_of(c)
    fails = []
    pre_value = None
    if c.pre:
        stored = got_pre.detach().cpu().double()
        if not bool(torch.isnan(stored[:, N:]).all()):
            fails.append("pre-activation pad columns written")
        stored = stored[:, :N]
        if c.p16:
            pre_value = stored                              # C is held to act(float(stored pre-activation))
    exp, exp_pre, mult = R.epilogue_ref(inp.P, prefill.double(), ldc, pre_value=pre_value, **kw)
    rows, cols, valid = R.targets(M, N, kw.get("c_win"))
    pos = (rows * ldc + cols)[valid]
    got = got_c.detach().cpu()
    # what the reference leaves untouched keeps its bits
    keep = torch.ones(got.numel(), dtype=torch.bool)
    keep[pos] = False
    bits = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    if not torch.equal(got.view(-1).view(bits)[keep], prefill.view(-1).view(bits)[keep]):
        fails.append("wrote outside its elements")
    g, e = got.double().view(-1)[pos], exp.view(-1)[pos]
    err = None
    if c.c16:
        r = _bf16_bar(g, e)
        if not r <= 1.0:
            fails.append(f"bf16 C {r:.3g} of one ulp")
    else:
        rel, err = _rel(g, e), elem_err(g, e)
        if not rel < TOL:
            fails.append(f"C max-norm {rel:.3g}")
        if not err < 1.0:
            fails.append(f"C elem_err {err:.3g}")
    if c.pre:
        if c.p16:
            r = _bf16_bar(stored, exp_pre)
            if not r <= 1.0:
                fails.append(f"bf16 pre-activation {r:.3g} of one ulp")
        else:
            rel, perr = _rel(stored, exp_pre), elem_err(stored, exp_pre)
            if not (rel < TOL and perr < 1.0):
                fails.append(f"pre-activation max-norm {rel:.3g} elem_err {perr:.3g}")
    if mult is not None and id(mult) not in _checked_masks:
        _checked_masks.add(id(mult))
        frac = float((mult[valid] == 0).double().mean())
        band = max(0.03, 4.0 * (DROP_P * (1.0 - DROP_P) / int(valid.sum())) ** 0.5)     # four sigma where elements are few
        if not abs(frac - DROP_P) < band:
            fails.append(f"dropped fraction {frac:.3f}")
    return fails, err
