"""Cases and references of the sequence-tile conv kernels (csrc/conv_seq.hip forward and d-input, csrc/conv_dw_seq.hip weight
gradient), CPU only.  The case lists are built at import time by asking the library what it admits and how it chunks a sequence
(tecm_conv_{fwd,dx,dw}_supported, tecm_conv_{fwd,dx}_tile_steps: pure host arithmetic); nothing here mirrors that arithmetic.

Every case is (B, Lc, N, cin, ld_in, Cout, f32).  Per kernel: one axis at a time from the two production bases, then a seeded
sample of the full admitted product.  A shape the predicate refuses goes to the *_REFUSED list instead.

Inputs: `exact_inputs` makes every partial sum a small multiple of 1/2, so a correct kernel returns the fp64 reference bit for
bit in any summation order; `random_inputs` are N(0, 1) with the a-priori element-wise bar of fp32 accumulation (`bar`).
References: torch's conv1d / conv1d_input / conv1d_weight in float64 on the sequence-major view."""
import itertools
import random
import zlib
from collections import namedtuple

import torch

Case = namedtuple("Case", "B Lc N cin ld_in Cout f32")
KS = (3, 5, 7)
SEED = 20240607                                            # of the sampled shapes
NSAMPLE = 24                                               # per kernel (12 per precision)
MAX_SEQ = 21                                               # B * N of a GPU case: the fp64 reference stays milliseconds

LCS = (8, 16, 24, 32, 40, 48, 56, 72, 88, 96, 104)            # 72: the forward's last chunk of 24 steps
NS = (1, 2, 3, 4, 5, 7)                                    # every remainder of the 4-node tile, and less than one tile
BS = (1, 3)
# the production blocks: block 1 reads the padded spatial output (22 channels at a pitch of 24), block 2 the first block's 64
BASES = (Case(2, 48, 5, 22, 24, 64, False), Case(1, 24, 7, 64, 64, 128, False))
FWD_COUT = (32, 64, 96, 128)
FWD_LD = (8, 16, 24, 40, 64, 72, 128)
FWD_F32_EDGE_LC = (24, 32, 40, 48)                         # where the fp32 forward's LDS limit on ld_in moves
DX_COUT = (64, 128, 192, 256, 448)
DX_COUT_LC8 = {False: (512, 768), True: (256,)}            # widths that only one 8-step tile holds, by f32
DX_LD = (4, 8, 24, 28, 32, 36, 64)
DW_PAIRS = ((64, 128), (24, 64), (64, 64), (24, 128))      # (ld_in, Cout) of TECM_DW_SHAPES
DW_LCS = (4, 8, 20, 24, 28, 44, 48, 52, 100)
DW_BLOCKS = ("1", "2", None)                               # TECM_CONV_DW_BLOCKS; None: unset = one block per CU
DW_TCMAX = 24                                              # csrc/conv_dw_seq.hip walks fixed chunks of 24 steps


def _h():
    import os
    from tecmollm import _lib
    if not os.path.exists(_lib.LIB_PATH):                  # as tests/test_host.py::built_lib
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def fwd_ok(c):
    return _h().tecm_conv_fwd_supported(c.Lc, c.Cout, c.ld_in, int(c.f32)) == 1


def dx_ok(c):
    return _h().tecm_conv_dx_supported(c.Lc, c.Cout, c.ld_in, int(c.f32)) == 1


def dw_ok(c):
    return _h().tecm_conv_dw_supported(c.Lc, c.Cout, c.ld_in) == 1


def fwd_tc(c):
    return _h().tecm_conv_fwd_tile_steps(c.Lc, c.Cout, c.ld_in, int(c.f32))


def dx_tc(c):
    return _h().tecm_conv_dx_tile_steps(c.Lc, c.Cout, c.ld_in, int(c.f32))


def chunks(Lc, tc):
    """The chunk lengths of a sequence walked in tiles of tc steps."""
    return [min(tc, Lc - t0) for t0 in range(0, Lc, tc)]


def plan(kind, c):
    return chunks(c.Lc, {"fwd": fwd_tc, "dx": dx_tc, "dw": lambda _c: min(DW_TCMAX, _c.Lc)}[kind](c))


def fwd_f32_max_ld(Lc, Cout=64):
    """The largest ld_in the fp32 forward admits at Lc, by asking."""
    return max(ld for ld in range(8, 129, 8) if _h().tecm_conv_fwd_supported(Lc, Cout, ld, 1) == 1)


def case_id(c):
    return f"B{c.B}_L{c.Lc}_N{c.N}_ci{c.cin}_ld{c.ld_in}_co{c.Cout}_{'fp32' if c.f32 else 'bf16'}"


def _cins(ld_in, offsets):
    return sorted({max(1, ld_in - o) if o is not None else 1 for o in offsets})


def _with_ld(base, ld):
    return base._replace(ld_in=ld, cin=max(1, ld - (base.ld_in - base.cin)))


def _sweeps(kind, base):
    out = []
    if kind == "dw":
        out += [base._replace(ld_in=ld, cin=max(1, ld - (base.ld_in - base.cin)), Cout=co) for ld, co in DW_PAIRS]
        out += [base._replace(Lc=L) for L in DW_LCS]
        out += [base._replace(cin=ci) for ci in _cins(base.ld_in, (None, 2, 0))]
    else:
        out += [base._replace(Lc=L) for L in LCS]
        if kind == "fwd":
            out += [base._replace(Cout=co) for co in FWD_COUT]
            lds = list(FWD_LD)
            if base.f32:
                for L in FWD_F32_EDGE_LC:
                    out.append(_with_ld(base._replace(Lc=L), fwd_f32_max_ld(L, base.Cout)))
            out += [_with_ld(base, ld) for ld in lds]
            out += [base._replace(cin=ci) for ci in _cins(base.ld_in, (None, 7, 2, 0))]
        else:
            out += [base._replace(Cout=co) for co in DX_COUT]
            out += [base._replace(Lc=8, Cout=co) for co in DX_COUT_LC8[base.f32]]
            out += [_with_ld(base, ld) for ld in DX_LD]
            out += [base._replace(cin=ci) for ci in _cins(base.ld_in, (None, 2, 0))]
    out += [base._replace(N=n) for n in NS]
    out += [base._replace(B=b) for b in BS]
    return out


def _product(kind, f32):
    if kind == "fwd":
        lds = sorted(set(FWD_LD) | ({fwd_f32_max_ld(L) for L in FWD_F32_EDGE_LC} if f32 else set()))
        shapes = [(L, ld, co, o) for L in LCS for ld in lds for co in FWD_COUT for o in (None, 7, 2, 0)]
    elif kind == "dx":
        shapes = [(L, ld, co, o) for L in LCS for ld in DX_LD for co in DX_COUT + (DX_COUT_LC8[f32] if L == 8 else ())
                  for o in (None, 2, 0)]
    else:
        shapes = [(L, ld, co, o) for L in DW_LCS for ld, co in DW_PAIRS for o in (None, 2, 0)]
    for (L, ld, co, o), n, b in itertools.product(shapes, NS, BS):
        yield Case(b, L, n, 1 if o is None else max(1, ld - o), ld, co, f32)


def _build(kind):
    ok = {"fwd": fwd_ok, "dx": dx_ok, "dw": dw_ok}[kind]
    sweep, sample, refused = [], [], []

    def put(c, where):
        assert c.B * c.N <= MAX_SEQ and 1 <= c.cin <= c.ld_in
        dst = where if ok(c) else refused
        if c not in sweep and c not in sample and c not in refused:
            dst.append(c)

    for f32 in (False, True):
        for base in BASES:
            for c in _sweeps(kind, base._replace(f32=f32)):
                put(c, sweep)
    rng = random.Random(SEED + {"fwd": 0, "dx": 1, "dw": 2}[kind])
    for f32 in (False, True):
        admitted = [c for c in _product(kind, f32) if ok(c)]
        n0 = len(sample)
        while len(sample) < n0 + NSAMPLE // 2:
            put(rng.choice(admitted), sample)
    return sweep, sample, refused


FWD_SWEEP, FWD_SAMPLE, FWD_REFUSED = _build("fwd")
DX_SWEEP, DX_SAMPLE, DX_REFUSED = _build("dx")
DW_SWEEP, DW_SAMPLE, DW_REFUSED = _build("dw")
FWD_CASES, DX_CASES, DW_CASES = FWD_SWEEP + FWD_SAMPLE, DX_SWEEP + DX_SAMPLE, DW_SWEEP + DW_SAMPLE
CASES = {"fwd": FWD_CASES, "dx": DX_CASES, "dw": DW_CASES}
SWEEPS = {"fwd": FWD_SWEEP, "dx": DX_SWEEP, "dw": DW_SWEEP}


def refusal_grid():
    """Shapes every launcher must refuse before any launch: (kind, Case), beyond what the sweeps already found refused."""
    b1, b2 = BASES
    grid = [("fwd", b1._replace(Lc=20)), ("fwd", b1._replace(Lc=44, f32=True)), ("dx", b1._replace(Lc=20)),
            ("dx", b2._replace(Lc=12, f32=True)), ("dw", b1._replace(Lc=6)), ("dw", b2._replace(Lc=22, f32=True)),
            ("fwd", b2._replace(Cout=160)), ("fwd", b2._replace(Cout=160, f32=True)),
            ("dx", _with_ld(b2, 68)), ("dx", _with_ld(b2, 68)._replace(f32=True)),
            ("dx", Case(1, 16, 4, 64, 64, 256, True)),
            ("dw", b2._replace(ld_in=32, cin=32)), ("dw", b2._replace(Cout=96)), ("dw", b1._replace(Cout=192, f32=True))]
    for L in LCS:                                          # the first ld_in above each fp32 forward limit
        ld = fwd_f32_max_ld(L) + 8
        if ld <= 128:
            grid.append(("fwd", Case(1, L, 4, ld, ld, 64, True)))
    grid += [("fwd", c) for c in FWD_REFUSED] + [("dx", c) for c in DX_REFUSED] + [("dw", c) for c in DW_REFUSED]
    return grid


# ------------------------------------------------------------------------------------------------------------ inputs
_WIDE = torch.tensor([-2.0, -1.0, 0.0, 1.0, 2.0])
_HALF = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0])
PAD_FILL = 1024.0                                          # input slack and padding columns: exact, and loud in an exact result


def _seed(kind, c, salt):
    return (zlib.crc32(repr((kind, tuple(int(v) for v in c))).encode()) + salt) % (2 ** 31)


def _pick(vals, shape, g):
    return vals[torch.randint(0, len(vals), shape, generator=g)]


def _terms(kind, c):
    """Accumulated terms of one output element, per kernel size (forward: + the bias) or overall."""
    if kind == "fwd":
        return [k * c.cin + 1 for k in KS]
    return 15 * c.Cout if kind == "dx" else c.B * c.Lc * c.N


def make_inputs(kind, c, exact, salt=0):
    """fp32 CPU tensors holding the values the kernel sees (bf16-representable in bf16 mode):
    fwd: x (B, Lc, N, ld_in; columns cin.. = PAD_FILL), ws [(Cout, cin, k)], bias (3 Cout);  dx: dy (B, Lc, N, 3 Cout), ws;
    dw: x as fwd, dy."""
    g = torch.Generator().manual_seed(_seed(kind, c, salt))
    CT = 3 * c.Cout
    if exact:
        acts, wts = (_WIDE, _HALF) if (c.Lc // 4 + c.N) % 2 else (_HALF, _WIDE)
        kmax = max(_terms(kind, c)) if kind == "fwd" else _terms(kind, c)
        assert 2 * (2.0 * kmax + 4.0) < 2 ** 24             # every partial sum is a multiple of 1/2 the fp32 format holds
        rnd = lambda shape, vals: _pick(vals, shape, g)
    else:
        acts = wts = None
        q = (lambda t: t) if c.f32 else (lambda t: t.bfloat16().float())
        rnd = lambda shape, vals: q(torch.randn(*shape, generator=g))
    d = {}
    if kind in ("fwd", "dw"):
        x = torch.full((c.B, c.Lc, c.N, c.ld_in), PAD_FILL)
        x[..., :c.cin] = rnd((c.B, c.Lc, c.N, c.cin), acts)
        d["x"] = x
    if kind in ("dx", "dw"):
        d["dy"] = rnd((c.B, c.Lc, c.N, CT), acts if kind == "dx" else wts)
    if kind in ("fwd", "dx"):
        d["ws"] = [rnd((c.Cout, c.cin, k), wts) for k in KS]
    if kind == "fwd":
        d["bias"] = (torch.randint(-4, 5, (CT,), generator=g).float() if exact else torch.randn(CT, generator=g))
    return d


def _seq(t):                                               # (B, Lc, N, C) -> (B N, C, Lc) float64
    B, Lc, N, C = t.shape
    return t.double().permute(0, 2, 3, 1).reshape(B * N, C, Lc)


def _unseq(t, B, N):                                       # (B N, C, Lc) -> (B, Lc, N, C)
    S, C, Lc = t.shape
    return t.reshape(B, N, C, Lc).permute(0, 3, 1, 2).contiguous()


def reference(kind, c, d, dtype=torch.float64, absolute=False):
    """The operation in `dtype` on the CPU (absolute: on the absolute values -- the sum the error bar scales with).
    fwd: y (B, Lc, N, 3 Cout); dx: dinp (B, Lc, N, cin); dw: [dw3, dw5, dw7]."""
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    Co = c.Cout
    if kind == "fwd":
        xs = f(_seq(d["x"][..., :c.cin])).to(dtype)
        ys = [torch.nn.functional.conv1d(xs, f(w).to(dtype), f(d["bias"][j * Co:(j + 1) * Co]).to(dtype), padding=(k - 1) // 2)
              for j, (k, w) in enumerate(zip(KS, d["ws"]))]
        return _unseq(torch.cat(ys, dim=1), c.B, c.N)
    dys = f(_seq(d["dy"])).to(dtype)
    if kind == "dx":
        S = c.B * c.N
        ref = torch.zeros(S, c.cin, c.Lc, dtype=dtype)
        for j, (k, w) in enumerate(zip(KS, d["ws"])):
            ref += torch.nn.grad.conv1d_input((S, c.cin, c.Lc), f(w).to(dtype), dys[:, j * Co:(j + 1) * Co].contiguous(),
                                              padding=(k - 1) // 2)
        return _unseq(ref, c.B, c.N)
    xs = f(_seq(d["x"][..., :c.cin])).to(dtype)
    return [torch.nn.grad.conv1d_weight(xs, (Co, c.cin, k), dys[:, j * Co:(j + 1) * Co].contiguous(), padding=(k - 1) // 2)
            for j, k in enumerate(KS)]


def _flat(kind, v):
    return torch.cat([t.reshape(-1) for t in v]) if kind == "dw" else v


def term_count(kind, c, like):
    """K of every element of the (flattened, for dw) result `like`."""
    K = torch.empty_like(like, dtype=torch.float64)
    if kind == "fwd":
        for j, k in enumerate(_terms(kind, c)):
            K[..., j * c.Cout:(j + 1) * c.Cout] = k
    else:
        K.fill_(_terms(kind, c))
    return K


def half_ulp_bf16(v):
    """Half a bf16 ulp (8 significand bits) at the magnitude of v (float64)."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))      # |v| = m 2^e, m in [1/2, 1)
    return torch.ldexp(torch.ones_like(v), e - 9)


def bar(kind, c, d, ref=None, out_bf16=False):
    """|got - ref64| <= K 2^-24 conv(|x|, |w|) per element -- fp32 accumulation of K exactly formed products in any order --
    plus K 2^-125 where the products underflow (the flat floor: an element whose terms cancel or vanish exactly keeps it), plus
    half a bf16 ulp at the reference's magnitude (and the bound's, should it cross a binade) where the output is bf16."""
    mag = _flat(kind, reference(kind, c, d, absolute=True))
    K = term_count(kind, c, mag)
    b = K * 2.0 ** -24 * mag + K * 2.0 ** -125
    if out_bf16:
        b = b + half_ulp_bf16(_flat(kind, ref).abs() + b)
    return b


def ratio(kind, got, ref, b):
    """Largest error / bound over the elements (a pass is < = 1)."""
    return float(((_flat(kind, got).double() - _flat(kind, ref)).abs() / b).max())


# ------------------------------------------------------------------------------------------------ planted faults
def plant(kind, c, d, fault, tc):
    """The reference of `kind` with one fault of the named class planted -- what a subtly wrong kernel would return.  tc: the
    tile steps of the case (chunk boundaries at multiples of tc)."""
    Co, k7 = c.Cout, 7
    ref = reference(kind, c, d)
    if fault == "halo_nonzero":
        # the k = 7 branch's outermost tap at the first and last time step reads a 1 where the zero padding is
        if kind == "fwd":
            w = d["ws"][2].double()
            ref[:, 0, :, 2 * Co:] += w[:, :, 0].sum(1)
            ref[:, -1, :, 2 * Co:] += w[:, :, k7 - 1].sum(1)
        elif kind == "dx":
            w = d["ws"][2].double()
            ref[:, 0] += w[:, :, k7 - 1].sum(0)
            ref[:, -1] += w[:, :, 0].sum(0)
        else:
            dys = _seq(d["dy"])[:, 2 * Co:]
            ref[2][:, :, 0] += dys[:, :, 0].sum(0)[:, None]
            ref[2][:, :, k7 - 1] += dys[:, :, -1].sum(0)[:, None]
        return ref
    if fault == "batch_leak":
        # batch b + 1's first step (batch b's last step, for the d-input) is seen behind the last step of batch b
        assert c.B > 1
        if kind == "fwd":
            x, w = d["x"][..., :c.cin].double(), d["ws"][0].double()             # k = 3: tap 2 of step Lc - 1 reads step Lc
            ref[:-1, -1, :, :Co] += torch.einsum("bnc,oc->bno", x[1:, 0], w[:, :, 2])
        elif kind == "dx":
            dy, w = d["dy"][..., :Co].double(), d["ws"][0].double()              # dinp[t] takes dy[t + 1] * w[tau = 0]
            ref[:-1, -1] += torch.einsum("bno,oc->bnc", dy[1:, 0], w[:, :, 0])
        else:
            x, dy = d["x"][..., :c.cin].double(), d["dy"][..., :Co].double()      # dw3[tau = 2] += dy[b, Lc - 1] x[b + 1, 0]
            ref[0][:, :, 2] += torch.einsum("bno,bnc->oc", dy[:-1, -1], x[1:, 0])
        return ref
    if fault == "node_copy":
        assert c.N > 1
        if kind == "dw":                                                         # node N - 1 contributes node N - 2's rows
            d2 = dict(d)
            d2["x"] = d["x"].clone()
            d2["x"][:, :, -1] = d["x"][:, :, -2]
            return reference(kind, c, d2)
        ref[:, :, -1] = ref[:, :, -2]
        return ref
    if fault == "chunk_halo_zero":
        # behind the first chunk boundary the halo rows of the previous chunk are taken as zero
        assert tc < c.Lc
        if kind == "dw":                                                         # the chunk's x image lacks the step before it
            d2 = {"x": d["x"].clone(), "dy": d["dy"].clone()}
            full = reference(kind, c, d)
            d2["dy"][:, :tc] = 0                                                  # contributions of the second chunk on ...
            with_halo = reference(kind, c, d2)
            d2["x"][:, :tc] = 0
            without = reference(kind, c, d2)
            return [f - a + b for f, a, b in zip(full, with_halo, without)]
        d2 = dict(d)
        key = "x" if kind == "fwd" else "dy"
        d2[key] = d[key].clone()
        d2[key][:, :tc] = 0
        cut = reference(kind, c, d2)
        ref[:, tc:] = cut[:, tc:]
        return ref
    if fault == "weight_scaled":
        s = 1.0 + 2.0 ** -10
        if kind == "dw":
            ref[1][:, :, 2] *= s
            return ref
        d2 = dict(d)
        d2["ws"] = [w.double().clone() for w in d["ws"]]
        d2["ws"][1][:, :, 2] *= s
        return reference(kind, c, d2)
    raise ValueError(fault)


FAULTS = ("halo_nonzero", "batch_leak", "node_copy", "chunk_halo_zero", "weight_scaled")
