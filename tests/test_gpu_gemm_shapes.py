"""Every GEMM kernel family either side of its tile, vector, split and dispatch edges, against the fp64 statement of the
contract (tests/gemm_epilogue_ref.py; case table, inputs and the dispatch conditions it restates: tests/gemm_shape_cases.py;
comparison and bars: check_case of tests/gemm_epilogue_cases.py, unchanged).

One test per family loops over its shapes -- one ragged base shape swept one axis at a time through {edge - 1, edge,
edge + 1} of every tile edge, vector width and dispatch threshold of that axis, the 27 shapes around one tile corner, and for
the fp32 kernels the operand offsets and leading dimensions that select each loader instance -- and runs every shape through
the probes whose code depends on raggedness: alpha only; bias + tanh-GELU with a stored pre-activation + residual + dropout
with a non-zero seed word; split-K; the window scatter of C; a bf16 C.  Every operand sits in a buffer of exactly the size
the contract asks for, NaN around the matrix; C has NaN pad columns, a wider ldc and a non-zero c_off, and whatever the call
must not write is compared bit for bit.  Every case asserts the kernel the dispatcher picked (tecm_gemm_last_kernel), a
fallback included, or TecmError where the contract refuses the shape.  Two smaller tables follow: split counts up to 64 (all
three splitk_reduce_kernel instantiations, asked counts above the real one, a last split of one short K-tile) and
Conv1d-shaped window views of A against torch's conv1d.  Failing cases are collected and reported together; every test
prints its number of cases, the kernels seen and the largest parity.elem_err (bar: < 1) with -s.  Measured on an MI355X:
profiles/gemm_shapes.txt."""
import time

import pytest
import torch

from tests import gemm_epilogue_cases as T
from tests import gemm_shape_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _pack(mat, ld, off, dtype, dev):
    """A (rows, cols) matrix with leading dimension ld, off elements into a buffer that ends with its last element; NaN
    wherever the matrix is not."""
    rows, cols = mat.shape
    buf = torch.full((off + (rows - 1) * ld + cols,), float("nan"))
    buf[off + torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]] = mat
    return buf.to(dtype).to(dev)


class _Operands:
    """One shape's operands on the device, in the storage the family's layouts and the shape's offsets ask for."""

    def __init__(self, fam, s, inp, dev, x=None):
        self.lda, self.ldb = S.lds(fam, s)
        adt = torch.bfloat16 if fam.a16 else torch.float32
        bdt = torch.bfloat16 if fam.b16 else torch.float32
        if x is not None:                                                 # a window view: A is the source tensor itself
            self.A = _pack(x, self.lda, s.a_off, adt, dev)
        else:
            self.A = _pack(inp.A.t() if fam.km else inp.A, self.lda, s.a_off, adt, dev)
        self.B = _pack(inp.B.t() if fam.kn else inp.B, self.ldb, s.b_off, bdt, dev)
        self.bias, self.residual = inp.bias.to(dev), inp.residual.to(dev)


def _launch(ops, fam, s, inp, d, probe, dev, split_k=S.SPLIT_ASKED, a_win=None):
    """One ops.gemm call; returns (C buffer, its pre-fill, pre-activation buffer or None, kernel name)."""
    c = S.PROBES[probe]
    prefill = inp.prefill(c, s.c_off)
    C = prefill.to(dev)
    kw = dict(alpha=T.ALPHA, act=c.act, split_k=split_k if c.split else 1, bf16=fam.prec, a_off=s.a_off, b_off=s.b_off,
              c_off=s.c_off, a_layout=ops.A_KM if fam.km else ops.A_MK, b_layout=ops.B_KN if fam.kn else ops.B_NK)
    pre = None
    if a_win is not None:
        kw["a_win"] = ops.win(*a_win)
    if c.bias:
        kw["bias"] = d.bias
    if c.pre:
        pre = torch.full((s.M, inp.ld), float("nan"), device=dev)
        kw["preact"] = (pre, inp.ld)
    if c.drop:
        kw["out_drop"] = ops.drop(T.DROP_P, T.DROP_SEED, inp.drop_ld_win if c.cwin else inp.drop_ld)
    if c.res:
        kw["residual"] = (d.residual, inp.ld)
    if c.cwin:
        kw["c_win"] = ops.win(*inp.c_win)
    rec = ops.enable_gemm_timing()
    try:
        ops.gemm(s.M, s.N, s.K, d.A, d.lda, d.B, d.ldb, C, inp.ldc_of(c), **kw)
        name = rec[-1][0]
    finally:
        ops.disable_gemm_timing()
    return C, prefill, pre, name


class _Tally:
    def __init__(self, name):
        self.name, self.failures, self.cases, self.refused, self.worst, self.kernels = name, [], 0, 0, 0.0, set()
        self.t0 = time.perf_counter()

    def run(self, ops, _lib, fam, s, inp, d, probe, dev, expected, what, **kw):
        self.cases += 1
        try:
            C, prefill, pre, kernel = _launch(ops, fam, s, inp, d, probe, dev, **kw)
        except _lib.TecmError as e:
            self.failures.append(f"{what}: refused ({e})")
            return
        self.kernels.add(kernel)
        if kernel != expected:
            self.failures.append(f"{what}: ran {kernel}, expected {expected}")
        fails, err = S.check_shape(inp, S.PROBES[probe], C, pre, prefill, s.c_off)
        self.worst = max(self.worst, err or 0.0)
        self.failures += [f"{what}: {f}" for f in fails]

    def refuse(self, ops, _lib, fam, s, inp, d, dev, what, **kw):
        self.refused += 1
        try:
            _launch(ops, fam, s, inp, d, "bare", dev, **kw)
            self.failures.append(f"{what}: not refused")
        except _lib.TecmError:
            pass

    def done(self):
        torch.cuda.synchronize()
        print(f"\n{self.name}: {self.cases} cases, {self.refused} refused, largest elem_err {self.worst:.3g}, "
              f"{time.perf_counter() - self.t0:.1f} s, kernels {sorted(self.kernels)}")
        assert self.cases > 0
        assert not self.failures, f"{len(self.failures)} failing: " + "; ".join(self.failures)


def _pin(monkeypatch, ops, fam, dev):
    for var in T.ENV_SWITCHES:
        monkeypatch.delenv(var, raising=False)
    for var, val in fam.env.items():
        monkeypatch.setenv(var, val)
    monkeypatch.setattr(ops, "SEED_WORD", torch.tensor([T.SEED_WORD], device=dev, dtype=torch.int64))


def _tag(s, probe):
    extra = "".join(f" {k}={v}" for k, v in (("lda", s.lda), ("ldb", s.ldb), ("ldc", s.ldc)) if v is not None)
    extra += "".join(f" {k}={v}" for k, v in (("a_off", s.a_off), ("b_off", s.b_off)) if v)
    return f"{s.M}x{s.N}x{s.K}{extra} c_off={s.c_off} {probe}"


@pytest.mark.parametrize("name", [f.name for f in S.SHAPE_FAMILIES])
def test_every_shape_edge_matches_the_fp64_contract(dev, name, monkeypatch):
    from tecmollm import ops, _lib
    fam = S.SHAPE_FAMILY[name]
    _pin(monkeypatch, ops, fam, dev)
    tally = _Tally(name)
    for s in S.shapes(fam):
        inp = S.inputs_for(fam, s)
        d = _Operands(fam, s, inp, dev)
        for probe in S.probes_of(fam, s):
            expected = S.expected_kernel(fam, s, probe, inp.ldc_of(S.PROBES[probe]))
            tally.run(ops, _lib, fam, s, inp, d, probe, dev, expected, _tag(s, probe))
    for s in fam.refused:                                                 # refused by contract: nothing may be launched
        inp = S.inputs_for(fam, s)
        tally.refuse(ops, _lib, fam, s, inp, _Operands(fam, s, inp, dev), dev, _tag(s, "bare"))
    assert tally.refused == len(fam.refused)
    tally.done()


@pytest.mark.parametrize("name", list(S.SPLIT_FAMILIES))
def test_split_counts_up_to_64_meet_the_full_epilogue(dev, name, monkeypatch):
    from tecmollm import ops, _lib
    fam = S.SHAPE_FAMILY[name]
    _pin(monkeypatch, ops, fam, dev)
    tally = _Tally(f"{name} split-K sweep at {S.SPLIT_MN[0]} x {S.SPLIT_MN[1]}")
    reducers = set()
    for sc in S.split_cases(name):
        s = S.split_shape(sc)
        inp = S.inputs_for(fam, s)
        d = _Operands(fam, s, inp, dev)
        reducers.add(S.reducer(sc.real))
        for probe in S.SPLIT_PROBES:
            expected = S.expected_kernel(fam, s, probe, inp.ldc)
            tally.run(ops, _lib, fam, s, inp, d, probe, dev, expected, f"{_tag(s, probe)} asked {sc.asked} real {sc.real}",
                      split_k=sc.asked)
    print(f"\n{name}: splitk_reduce_kernel instantiations reached {sorted(r for r in reducers if r)}")
    assert reducers >= {4, 8, 16}
    tally.done()


@pytest.mark.parametrize("name", S.WIN_FAMILIES)
def test_conv1d_shaped_window_views_of_a_match_conv1d(dev, name, monkeypatch):
    from tecmollm import ops, _lib
    fam = S.win_family(name)
    _pin(monkeypatch, ops, fam, dev)
    tally = _Tally(f"{name} window views of A")
    for w in S.WIN_CASES:
        inp = S.win_inputs(w, fam.prec == 1)
        s = S.shape(w.B * w.Lout * w.nodes, S.WIN_N, w.taps * w.Cw, lda=w.Cw)
        d = _Operands(fam, s, inp, dev, x=inp.x)
        expected = S.win_expected(name, w)
        what = f"{s.M}x{s.N}x{s.K} taps {w.taps} stride {w.stride} Cw {w.Cw}"
        if expected is None:
            tally.refuse(ops, _lib, fam, s, inp, d, dev, what, a_win=S.win_geometry(w))
            continue
        for probe in ("bare", "loaded"):
            tally.run(ops, _lib, fam, s, inp, d, probe, dev, expected, f"{what} {probe}", a_win=S.win_geometry(w))
    tally.done()
