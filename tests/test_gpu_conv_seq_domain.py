"""GPU tests of the sequence-tile conv kernels (csrc/conv_seq.hip forward and d-input, csrc/conv_dw_seq.hip weight gradient) on
every kind of shape their predicates admit: tests/conv_seq_cases.py builds the cases by asking the library for its tile plans.

Exact inputs (every partial sum a small multiple of 1/2): the kernel returns the fp64 reference BIT FOR BIT, in bf16 and in fp32,
on every case.  N(0, 1) inputs, on the one-axis sweeps: |got - ref64| <= K 2^-24 conv(|x|, |w|) per element, the a-priori bound
of fp32 accumulation (cs.bar).  Every tensor a kernel touches is a 16-byte aligned view inside a larger buffer with 256 bytes
of slack either side: 1024.0 around inputs (exact, loud in an exact result), NaN around outputs (must still be NaN).

With TECM_CONV_DOMAIN_LOG=<file> the module writes one line per case -- shape, precision, the library's chunk plan, exact-equal
yes / no and, for the random-input cases, the largest error / bound of the kernel and of the one-thread float32 CPU convolution
of the same operands: profiles/conv_seq_domain.txt is such a run."""
import ctypes as C
import os

import pytest
import torch

from tests import conv_seq_cases as cs

pytestmark = pytest.mark.gpu
SLACK = 256                                                # bytes either side of every tensor
_REC = {}                                                  # (kind, case) -> fields of its profile line


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda")
    path = os.environ.get("TECM_CONV_DOMAIN_LOG")
    if path:
        with open(path, "w", encoding="utf-8") as f:
            f.write("# kernel shape plan(time steps per tile) exact-equal [largest error/bound on N(0,1): kernel, float32 CPU]\n")
            for (kind, c), r in _REC.items():
                f.write(f"{kind:3s} {cs.case_id(c):44s} plan={'+'.join(map(str, cs.plan(kind, c))):18s} "
                        f"exact={r.get('exact', '-'):3s}"
                        + (f" ratio_kernel={r['kernel']:.4f} ratio_cpu_f32={r['cpu']:.4f}" if "kernel" in r else "") + "\n")


def _ids(cases):
    return [cs.case_id(c) for c in cases]


class Guarded:
    """A tensor as a view inside a larger device buffer; inputs are snapshot for the unchanged check."""

    def __init__(self, shape, dtype, dev, fill, src=None):
        n = 1
        for s in shape:
            n *= s
        self.slack = SLACK // torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((n + 2 * self.slack,), fill, dtype=dtype, device=dev)
        self.t = self.buf[self.slack:self.slack + n].view(*shape)
        assert self.t.data_ptr() % 16 == 0
        if src is not None:
            self.t.copy_(src.to(dtype))
        self.before = self.buf.clone() if src is not None else None

    def check(self, what):
        if self.before is not None:
            assert torch.equal(self.buf, self.before), f"{what}: an input was written"
        else:
            s = self.slack
            assert bool(torch.isnan(self.buf[:s]).all()) and bool(torch.isnan(self.buf[-s:]).all()), f"{what}: slack written"
            assert not bool(torch.isnan(self.t).any()), f"{what}: unwritten or NaN elements inside the output"


def _inp(t, dev, dtype=torch.float32):
    return Guarded(tuple(t.shape), dtype, dev, cs.PAD_FILL, src=t)


def _out(shape, dev, dtype=torch.float32):
    return Guarded(shape, dtype, dev, float("nan"))


def _where(got, ref):
    bad = (got != ref).nonzero()
    return f"{len(bad)} wrong elements, first at {bad[:4].tolist()}: got {[float(got[tuple(i)]) for i in bad[:4]]}, " \
           f"want {[float(ref[tuple(i)]) for i in bad[:4]]}"


def run_fwd(c, d, dev, y_dtype=torch.float32):
    from tecmollm import ops
    x = _inp(d["x"], dev, torch.float32 if c.f32 else torch.bfloat16)
    ws = [_inp(w, dev) for w in d["ws"]]
    bias = _inp(d["bias"], dev)
    y = _out((c.B, c.Lc, c.N, 3 * c.Cout), dev, y_dtype)
    assert ops.conv_fwd_seq_ok(c.Lc, c.Cout, c.ld_in, f32=c.f32)
    ops.conv_fwd(x.t, ws[0].t, ws[1].t, ws[2].t, bias.t, y.t, c.B, c.Lc, c.N, c.Cout, c.cin, c.ld_in)
    torch.cuda.synchronize()
    for g in [x, bias, y] + ws:
        g.check(cs.case_id(c))
    return y.t.cpu()


def run_dx(c, d, dev):
    from tecmollm import ops
    dy = _inp(d["dy"], dev, torch.float32 if c.f32 else torch.bfloat16)
    ws = [_inp(w, dev) for w in d["ws"]]
    out = _out((c.B, c.Lc, c.N, c.ld_in), dev)
    assert ops.conv_dx_seq_ok(c.Lc, c.Cout, c.ld_in, f32=c.f32)
    ops.conv_dx(dy.t, ws[0].t, ws[1].t, ws[2].t, out.t, c.B, c.Lc, c.N, c.Cout, c.cin, c.ld_in)
    torch.cuda.synchronize()
    for g in [dy, out] + ws:
        g.check(cs.case_id(c))
    return out.t.cpu()


def run_dw(c, d, dev):
    """Through the C ABI with guarded outputs (ops.conv_dw allocates its own), one block per CU."""
    from tecmollm import _lib, ops
    dt = torch.float32 if c.f32 else torch.bfloat16
    x, dy = _inp(d["x"], dev, dt), _inp(d["dy"], dev, dt)
    nb = torch.cuda.get_device_properties(dev).multi_processor_count
    nws = _lib.lib().tecm_conv_dw_workspace(c.Cout, c.ld_in, nb)
    assert nws > 0 and ops.conv_dw_seq_ok(c.Lc, c.Cout, c.ld_in)
    ws = torch.empty(nws, device=dev)
    dws = [_out((c.Cout, c.cin, k), dev) for k in cs.KS]
    desc = _lib.TecmConvDw(inp=x.t.data_ptr(), dy=dy.t.data_ptr(), workspace=ws.data_ptr(), dw3=dws[0].t.data_ptr(),
                           dw5=dws[1].t.data_ptr(), dw7=dws[2].t.data_ptr(), B=c.B, Lc=c.Lc, N=c.N, Cout=c.Cout, Cin=c.cin,
                           ld_in=c.ld_in, num_blocks=nb)
    run = _lib.lib().tecm_conv_dw_f32 if c.f32 else _lib.lib().tecm_conv_dw_bf16
    _lib.check(run(C.byref(desc), _lib.stream_ptr()), "tecm_conv_dw")
    torch.cuda.synchronize()
    for g in [x, dy] + dws:
        g.check(cs.case_id(c))
    return [g.t.cpu() for g in dws], x, dy


def _cpu_f32_ratio(kind, c, d, ref, b):
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return cs.ratio(kind, cs.reference(kind, c, d, dtype=torch.float32), ref, b)
    finally:
        torch.set_num_threads(n)


def _exact(kind, c, got, ref):
    ok = torch.equal(cs._flat(kind, got).double(), cs._flat(kind, ref))
    _REC.setdefault((kind, c), {})["exact"] = "yes" if ok else "no"
    assert ok, f"{kind} {cs.case_id(c)} plan {cs.plan(kind, c)}: " + _where(cs._flat(kind, got).double(), cs._flat(kind, ref))


def _random(kind, c, d, got, ref, out_bf16=False):
    b = cs.bar(kind, c, d, ref, out_bf16=out_bf16)
    r = cs.ratio(kind, got, ref, b)
    if not out_bf16:
        _REC.setdefault((kind, c), {}).update(kernel=r, cpu=_cpu_f32_ratio(kind, c, d, ref, b))
    print(f"{kind} {cs.case_id(c)} plan {cs.plan(kind, c)}{' bf16 out' if out_bf16 else ''}: largest error / bound {r:.4f}")
    assert r <= 1.0, f"{kind} {cs.case_id(c)}: largest error / bound {r}"


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("c", cs.FWD_CASES, ids=_ids(cs.FWD_CASES))
def test_conv_fwd_returns_the_fp64_reference_bit_for_bit_on_exact_inputs(dev, c):
    d = cs.make_inputs("fwd", c, exact=True)
    ref = cs.reference("fwd", c, d)
    _exact("fwd", c, run_fwd(c, d, dev), ref)
    if not c.f32:                                          # the bf16 y: the same accumulators, rounded once
        y16 = run_fwd(c, d, dev, torch.bfloat16)
        want = ref.float().bfloat16()
        assert torch.equal(y16, want), _where(y16.double(), want.double())


@pytest.mark.parametrize("c", cs.FWD_SWEEP, ids=_ids(cs.FWD_SWEEP))
def test_conv_fwd_meets_the_elementwise_bar_on_random_inputs(dev, c):
    d = cs.make_inputs("fwd", c, exact=False)
    ref = cs.reference("fwd", c, d)
    _random("fwd", c, d, run_fwd(c, d, dev), ref)
    if not c.f32:
        _random("fwd", c, d, run_fwd(c, d, dev, torch.bfloat16), ref, out_bf16=True)


def _stats_cases():
    from tecmollm.functions import conv_block_y16
    out = []
    for Lc in (16, 32, 40):
        for N in (1, 3, 5):
            for cin, ld_in, Cout in ((22, 24, 64), (64, 64, 128), (22, 24, 32), (64, 64, 32), (22, 24, 96), (64, 64, 96)):
                if Cout in (64, 128) or conv_block_y16(Lc, N, Cout, ld_in):
                    out.append((Lc, N, cin, ld_in, Cout))
    return out


_STATS = _stats_cases()


@pytest.mark.parametrize("Lc,N,cin,ld_in,Cout", _STATS, ids=[f"L{s[0]}_N{s[1]}_ld{s[3]}_co{s[4]}" for s in _STATS])
def test_conv_fwd_statistics_on_every_k_loop_instantiation(dev, Lc, N, cin, ld_in, Cout):
    """TecmConvFwd::stats at 2, 4 and 5 row tiles and every remainder of the node tile: the fp64 comparison of
    tests/test_gpu_bf16.py::test_conv_fwd_hands_the_groupnorm_statistics_over (mean, rstd of the y it wrote: 1e-5 max-norm)."""
    from tecmollm import ops
    Bn, CT = 2, 3 * Cout
    g = torch.Generator().manual_seed(Lc * 100 + N)
    inp = torch.zeros(Bn, Lc, N, ld_in)
    inp[..., :cin] = torch.randn(Bn, Lc, N, cin, generator=g)
    inp16 = inp.bfloat16().to(dev)
    ws = [(torch.randn(Cout, cin, k, generator=g) * 0.2).to(dev) for k in cs.KS]
    bias = torch.randn(CT, generator=g).to(dev)
    y, y0 = _out((Bn, Lc, N, CT), dev, torch.bfloat16), _out((Bn, Lc, N, CT), dev, torch.bfloat16)
    stats = _out((Bn * N, 3, 2), dev)
    ops.conv_fwd(inp16, *ws, bias, y.t, Bn, Lc, N, Cout, cin, ld_in, stats=stats.t)
    ops.conv_fwd(inp16, *ws, bias, y0.t, Bn, Lc, N, Cout, cin, ld_in)
    torch.cuda.synchronize()
    for t in (y, y0, stats):
        t.check("stats")
    assert torch.equal(y.t, y0.t)
    yd = y.t.double().view(Bn, Lc, N, 3, Cout).permute(0, 2, 3, 1, 4).reshape(Bn * N, 3, -1)
    mean, var = yd.mean(-1), yd.var(-1, unbiased=False)
    rel = lambda a, b: float((a.double() - b).abs().max() / (b.abs().max() + 1e-30))
    assert rel(stats.t[..., 0], mean) < 1e-5 and rel(stats.t[..., 1], 1.0 / torch.sqrt(var + 1e-5)) < 1e-5


def test_conv_fwd_refuses_statistics_it_cannot_compute(dev):
    """A sequence longer than one tile, an fp32 y and the fp32 kernel: the call with `stats` is refused, nothing is written."""
    from tecmollm import TecmError, ops
    c = cs.BASES[0]._replace(Lc=56)
    d = cs.make_inputs("fwd", c, exact=True)
    ws = [w.to(dev) for w in d["ws"]]
    bias = d["bias"].to(dev)
    for x_dt, y_dt, Lc in ((torch.bfloat16, torch.bfloat16, 56), (torch.bfloat16, torch.float32, 48), (torch.float32, torch.float32, 48)):
        y, stats = _out((c.B, Lc, c.N, 3 * c.Cout), dev, y_dt), _out((c.B * c.N, 3, 2), dev)
        with pytest.raises(TecmError):
            ops.conv_fwd(d["x"][:, :Lc].contiguous().to(x_dt).to(dev), *ws, bias, y.t, c.B, Lc, c.N, c.Cout, c.cin, c.ld_in,
                         stats=stats.t)
        torch.cuda.synchronize()
        assert bool(torch.isnan(y.buf).all()) and bool(torch.isnan(stats.buf).all())


# ------------------------------------------------------------------------------------------------------------ d-input
@pytest.mark.parametrize("c", cs.DX_CASES, ids=_ids(cs.DX_CASES))
def test_conv_dx_returns_the_fp64_reference_bit_for_bit_on_exact_inputs(dev, c):
    d = cs.make_inputs("dx", c, exact=True)
    got = run_dx(c, d, dev)
    _exact("dx", c, got[..., :c.cin], cs.reference("dx", c, d))
    assert not bool(got[..., c.cin:].any()), "the padding columns cin .. ld_in are exactly zero"


@pytest.mark.parametrize("c", cs.DX_SWEEP, ids=_ids(cs.DX_SWEEP))
def test_conv_dx_meets_the_elementwise_bar_on_random_inputs(dev, c):
    d = cs.make_inputs("dx", c, exact=False)
    got = run_dx(c, d, dev)
    _random("dx", c, d, got[..., :c.cin], cs.reference("dx", c, d))
    assert not bool(got[..., c.cin:].any())


# ---------------------------------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("c", cs.DW_CASES, ids=_ids(cs.DW_CASES))
def test_conv_dw_returns_the_fp64_reference_bit_for_bit_on_exact_inputs(dev, c, monkeypatch):
    """... whatever finite values the input's padding columns hold, on a second run and with every TECM_CONV_DW_BLOCKS."""
    from tecmollm import ops
    d = cs.make_inputs("dw", c, exact=True)
    d["x"][..., c.cin:] = torch.randn(c.B, c.Lc, c.N, c.ld_in - c.cin, generator=torch.Generator().manual_seed(c.Lc)) * 100
    ref = cs.reference("dw", c, d)
    got, x, dy = run_dw(c, d, dev)
    _exact("dw", c, got, ref)
    try:
        for blocks in cs.DW_BLOCKS + (None,):              # unset twice: a second run
            if blocks is None:
                monkeypatch.delenv("TECM_CONV_DW_BLOCKS", raising=False)
            else:
                monkeypatch.setenv("TECM_CONV_DW_BLOCKS", blocks)
            ops._cu_count.clear()
            again = ops.conv_dw(x.t, dy.t, c.B, c.Lc, c.N, c.Cout, c.cin, c.ld_in)
            torch.cuda.synchronize()
            for a, w in zip(again, got):
                assert torch.equal(a.cpu(), w), f"TECM_CONV_DW_BLOCKS={blocks}"
    finally:
        ops._cu_count.clear()
    x.check("dw")
    dy.check("dw")


@pytest.mark.parametrize("c", cs.DW_SWEEP, ids=_ids(cs.DW_SWEEP))
def test_conv_dw_meets_the_elementwise_bar_on_random_inputs(dev, c):
    d = cs.make_inputs("dw", c, exact=False)
    got, _, _ = run_dw(c, d, dev)
    _random("dw", c, d, got, cs.reference("dw", c, d))
