"""The reduction kernels on every route, shape edge and output mode (tables, families and references: tests/reduction_cases.py;
the same tables without a GPU: tests/test_host_reduction_cases.py).

Column sums (csrc/colsum.hip) go through the C ABI directly, because tecmollm.ops pins ldo = C: every case writes a window of
a larger sentinel-filled tensor (ldo > C, rows before and after), into a NaN-filled output and workspace, three times, and
the three results must agree bit for bit.  The EXACT family (integer-valued inputs) is held to the int64 sum under
torch.equal; the REAL family (N(0, 1)) to the forward error bound of any summation order.  The LayerNorm / GroupNorm
partial rows, the Huber loss, the clip norm with the AdamW update and the parameter checksum follow, each at both sides of
its launcher's block cap.

With TECM_REDUCTION_LOG=<file> the module writes one row per case -- route, worst ratio to its bar, whether the three
launches agreed, a hash of the output: profiles/reduction_domain.txt is such a run.  TECM_REDUCTION_PARENT_LIB=<library> names
another build of the library (the parent commit's): the same column-sum calls go through it as well (colsum_hashes below) and
the record says whether the outputs agree bit for bit."""
import ctypes as C
import hashlib
import math
import os

import numpy as np
import pytest
import torch

from tests import hard_inputs as hi
from tests import reduction_cases as rc

pytestmark = pytest.mark.gpu

TOL = 2e-4                 # tests/test_gpu_ops.py: the GroupNorm kernels against float64
TOL_BF16 = 5e-3            # ... a bf16 dy
_REC = []                  # (group, case, route, worst ratio to the bar, the three launches agreed, output hash)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield torch.device("cuda")
    path = os.environ.get("TECM_REDUCTION_LOG")
    if path:
        other = os.environ.get("TECM_REDUCTION_PARENT_LIB")
        parent = colsum_hashes(C.CDLL(other), torch.device("cuda")) if other else {}
        with open(path, "w", encoding="utf-8") as f:
            f.write("# group case | route | worst ratio to the bar (<= 1 passes; column sums: the N(0, 1) family, the integer-valued one is held to torch.equal) | three launches into NaN-filled outputs "
                    "bit-identical | SHA-256 (first 16 hex) of the outputs | the same calls through the parent commit's library\n")
            for group, case, route, ratio, agree, digest in _REC:
                same = "-" if digest == "-" or not parent else ("identical" if parent.get(f"{group}/{case}") == digest else "DIFFERENT")
                f.write(f"{group:10s} {case:34s} | {route:44s} | {ratio:9.3g} | {agree:5s} | {digest:16s} | {same}\n")
            routes = sorted({r for g, _, r, *_ in _REC if g in ("colsum", "batch", "twin")})
            f.write("# column-sum routes reached (first stage, second-stage waves): "
                    + ", ".join(sorted({f"{r.split()[0]}/{r.split('waves=')[1].split()[0]}" for r in routes})) + "\n")
            if parent:
                n = sum(1 for g, c, _, _, _, d in _REC if d != "-")
                bad = sum(1 for g, c, _, _, _, d in _REC if d != "-" and parent.get(f"{g}/{c}") != d)
                f.write(f"# outputs compared with the parent commit's library: {n}; differing: {bad}\n")


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """A lost context fails every later launch the same way: end the run at the test that lost it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU context is lost after this test: {e}", returncode=3)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(_bits(t).cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def _drop(p, drop_ld):
    from tecmollm import ops
    return ops.drop(p, rc.MASK_SEED, drop_ld) if p > 0 else ops.NO_DROP


def _stream():
    from tecmollm._lib import stream_ptr
    return C.c_void_p(stream_ptr())


# ------------------------------------------------------------------------------------------------ column sums
def colsum_launch(h, c, buf, out0, twin=None, ld_twin=0):
    """One tecm_colsum / tecm_colsum_twin call of case `c` through library handle `h` (every argument as an explicit
    ctypes value, so that a plain ctypes.CDLL serves): the (nseg, C) window at row 1, column 1 of a sentinel-filled
    (nseg + 2, C + 3) tensor, NaN where the call does not accumulate, and a NaN-filled workspace.  Returns the whole tensor."""
    ldo = c.C + 3
    big = torch.full((c.nseg + 2, ldo), rc.SENTINEL, device=buf.device)
    big[1:1 + c.nseg, 1:1 + c.C] = out0.to(buf.device)
    ws = torch.full((1024 * c.nseg * c.C,), rc.NAN, device=buf.device)
    spec = _drop(c.p, getattr(c, "drop_ld", c.ld))
    args = [C.c_void_p(buf.data_ptr() + 4 * getattr(c, "off", 0)), C.c_int64(c.ld), C.c_int64(c.outer), C.c_int64(c.inner),
            C.c_int32(c.nseg), C.c_int32(c.C), C.c_void_p(big.data_ptr() + 4 * (ldo + 1)), C.c_int64(ldo),
            C.c_int32(getattr(c, "acc", 0)), C.c_float(getattr(c, "scale", 1.0)), C.byref(spec), C.c_void_p(ws.data_ptr())]
    if twin is None:
        code = h.tecm_colsum(*args, _stream())
    else:
        code = h.tecm_colsum_twin(*args, C.c_void_p(twin.data_ptr()), C.c_int64(ld_twin), _stream())
    return code, big


def _window(big, c):
    return big[1:1 + c.nseg, 1:1 + c.C]


def _sentinel_kept(big, c):
    outside = torch.ones_like(big, dtype=torch.bool)
    outside[1:1 + c.nseg, 1:1 + c.C] = False
    return bool((big[outside] == rc.SENTINEL).all())


def batch_launch(h, mats, b):
    """tecm_colsum_batch of the case's matrices into rows of a NaN-filled (nbuf, C) tensor, NaN-filled workspace."""
    out = torch.full((b.nbuf, b.C), rc.NAN, device=mats[0].device)
    ws = torch.full((max(1024, 256 * b.nbuf) * b.C,), rc.NAN, device=out.device)
    ins = (C.c_void_p * b.nbuf)(*[m.data_ptr() for m in mats])
    outs = (C.c_void_p * b.nbuf)(*[out.data_ptr() + 4 * b.C * i for i in range(b.nbuf)])
    code = h.tecm_colsum_batch(ins, outs, C.c_int32(b.nbuf), C.c_int64(b.C), C.c_int64(b.rows), C.c_int32(b.C),
                               C.c_void_p(ws.data_ptr()), _stream())
    return code, out


def _twin_tensor(t, device):
    return torch.full((t.outer * t.nseg * t.inner, t.ld_twin), rc.SENTINEL, device=device, dtype=torch.bfloat16)


def colsum_hashes(h, device):
    """{"group/case": digest} of the REAL-family outputs of every column-sum, twin and batch case through handle `h`: what
    two builds of the library are compared by."""
    out = {}
    for c in rc.COLSUM:
        code, big = colsum_launch(h, c, rc.colsum_buffer(c, "real").to(device), rc.colsum_out0(c, "real"))
        assert code == 0, c.name
        out[f"colsum/{c.name}"] = _digest(big)
    for t in rc.TWINS:
        tw = _twin_tensor(t, device)
        code, big = colsum_launch(h, t, rc.colsum_buffer(_as_colsum(t), "real").to(device), torch.full((t.nseg, t.C), rc.NAN), tw, t.ld_twin)
        assert code == 0, t.name
        out[f"twin/{t.name}"] = _digest(big, tw)
    for b in rc.BATCH:
        code, res = batch_launch(h, rc.batch_matrices(b, "real", device), b)
        assert code == 0, b.name
        out[f"batch/{b.name}"] = _digest(res)
    return out


def _as_colsum(t):
    return rc.Colsum(t.name, t.C, t.ld, 0, t.outer, t.inner, t.nseg, t.p, t.ld, 1.0, 0, "")


def test_column_sums_exact_and_real_on_every_route(dev):
    from tecmollm import ops
    h = ops.lib()
    for c in rc.COLSUM:
        assert ops.colsum_path(c.ld, c.outer, c.inner, c.nseg, c.C, 4 * (c.off % 4), 0) == c.route, c.name
        mult = rc.colsum_mult(c)
        mult = None if mult is None else mult.to(dev)
        # EXACT: the int64 sum, no tolerance
        buf, out0 = rc.colsum_buffer(c, "exact").to(dev), rc.colsum_out0(c, "exact")
        assert (buf.data_ptr() + 4 * c.off) % 16 == 4 * (c.off % 4)
        code, big = colsum_launch(h, c, buf, out0)
        assert code == 0, (c.name, ops.lib().tecm_last_error())
        ref = rc.colsum_ref_exact(rc.colsum_values(buf, c), mult, c, out0)
        exact = torch.equal(_window(big, c), ref)
        assert exact, (c.name, "exact", float((_window(big, c) - ref).abs().max()))
        assert _sentinel_kept(big, c), c.name
        # REAL: the bound of any order, and three launches bit for bit
        buf, out0 = rc.colsum_buffer(c, "real").to(dev), rc.colsum_out0(c, "real")
        bigs = [colsum_launch(h, c, buf, out0)[1] for _ in range(3)]
        ref, bound = rc.colsum_ref_real(rc.colsum_values(buf, c), mult, c, out0)
        ratio = rc.real_ratio(_window(bigs[0], c), ref, bound)
        agree = all(torch.equal(_bits(b), _bits(bigs[0])) for b in bigs[1:])
        _REC.append(("colsum", c.name, c.route, ratio, "yes" if agree else "NO", _digest(bigs[0])))
        assert ratio <= 1.0, (c.name, "real", ratio)
        assert agree and _sentinel_kept(bigs[0], c), c.name


def test_column_sum_twin_is_the_rounded_masked_input(dev):
    from tecmollm import ops
    h = ops.lib()
    for t in rc.TWINS:
        c = _as_colsum(t)
        route = ops.colsum_path(t.ld, t.outer, t.inner, t.nseg, t.C)
        mult = rc.colsum_mult(c)
        for family in ("exact", "real"):
            buf = rc.colsum_buffer(c, family).to(dev)
            nan0 = torch.full((t.nseg, t.C), rc.NAN)
            runs = []
            for _ in range(3):
                tw = _twin_tensor(t, dev)
                code, big = colsum_launch(h, t, buf, nan0, tw, t.ld_twin)
                assert code == 0, (t.name, ops.lib().tecm_last_error())
                runs.append((big, tw))
            big, tw = runs[0]
            vals = rc.colsum_values(buf, c)
            masked = buf[:c.rows * c.ld].view(c.rows, c.ld)[:, :c.C] * (1.0 if mult is None else mult.to(dev))
            assert torch.equal(tw[:, :t.C], masked.bfloat16()), (t.name, family)
            assert bool((tw[:, t.C:] == rc.SENTINEL).all()), (t.name, family)            # the twin's padding columns
            plain = colsum_launch(h, c, buf, nan0)[1]
            assert torch.equal(_bits(big), _bits(plain)), (t.name, family)               # the sums of tecm_colsum, same bits
            if family == "exact":
                assert torch.equal(_window(big, c), rc.colsum_ref_exact(vals, None if mult is None else mult.to(dev), c, nan0)), t.name
            else:
                ref, bound = rc.colsum_ref_real(vals, None if mult is None else mult.to(dev), c, nan0)
                ratio = rc.real_ratio(_window(big, c), ref, bound)
                agree = all(torch.equal(_bits(a), _bits(big)) and torch.equal(_bits(b), _bits(tw)) for a, b in runs[1:])
                _REC.append(("twin", t.name, route, ratio, "yes" if agree else "NO", _digest(big, tw)))
                assert ratio <= 1.0 and agree and _sentinel_kept(big, c), (t.name, ratio, agree)
    for Cn, ld, ld_twin in rc.TWIN_REFUSED:                                           # no float4 first stage: refused, nothing written
        c = rc.Colsum("refused", Cn, ld, 0, 37, 5, 3, 0.0, ld, 1.0, 0, "")
        tw = torch.full((c.rows, ld_twin), rc.SENTINEL, device=dev, dtype=torch.bfloat16)
        code, big = colsum_launch(h, rc.Twin("refused", Cn, ld, 37, 5, 3, 0.0, ld_twin), rc.colsum_buffer(c, "exact").to(dev),
                                  torch.full((3, Cn), rc.SENTINEL), tw, ld_twin)
        assert code < 0 and bool((tw == rc.SENTINEL).all()) and bool((big == rc.SENTINEL).all()), (Cn, ld)


def test_column_sum_batch_rows_are_colsum_of_each_matrix(dev):
    from tecmollm import ops
    h = ops.lib()
    for b in rc.BATCH:
        assert ops.colsum_path(b.C, b.rows, 1, 1, b.C, b.best_misalign, b.nbuf) == b.route, b.name
        for family in ("exact", "real"):
            mats = rc.batch_matrices(b, family, dev)
            runs = [batch_launch(h, mats, b) for _ in range(3 if family == "real" else 1)]
            assert all(code == 0 for code, _ in runs), (b.name, ops.lib().tecm_last_error())
            out = runs[0][1]
            single = torch.stack([ops.colsum(m, b.C, b.rows, 1, 1, b.C)[0] for m in mats])    # the header's contract, bit for bit
            assert torch.equal(_bits(out), _bits(single)), (b.name, family)
            via_ops = ops.colsum_batch(mats, b.rows, b.C)
            assert torch.equal(_bits(out), _bits(via_ops)), (b.name, family)
            stack = torch.stack(mats)
            if family == "exact":
                assert torch.equal(out, stack.to(torch.int64).sum(1).float()), b.name
            else:
                ref = stack.double().sum(1)
                bound = rc.gamma_n(b.rows) * stack.double().abs().sum(1) + rc.ulp32(ref)
                ratio = rc.real_ratio(out, ref, bound)
                agree = all(torch.equal(_bits(o), _bits(out)) for _, o in runs[1:])
                _REC.append(("batch", b.name, b.route, ratio, "yes" if agree else "NO", _digest(out)))
                assert ratio <= 1.0 and agree, (b.name, ratio, agree)


# ------------------------------------------------------------------------------------------------ LayerNorm partials
def _ln_check(ops, dev, M, D, variant="plain"):
    x, gamma, dy, dy2 = rc.ln_case_inputs(M, D, dev)
    y, st = torch.empty(M, D, device=dev), torch.full((M, 2), rc.NAN, device=dev)
    ops.layernorm_fwd(x, D, gamma, torch.zeros(D, device=dev), y, D, st, M, D)
    arg, kw, dy_eff = dy, {}, dy
    if variant == "add32":                     # a second gradient stream under a p = 0.5 mask: still integer-valued
        mult = rc.colsum_mult(None, rows=M, cols=D, drop_ld=D, p=0.5).to(dev)
        kw, dy_eff = {"add": (dy2, D, _drop(0.5, D))}, dy + mult * dy2
    elif variant == "dy16":
        arg = dy.bfloat16()
    elif variant == "seq_major":               # the sequence-major bf16 dy with its mask, index = the time-major one
        B, T, N = rc.LN_VARIANT_SHAPE[2]
        mult = rc.colsum_mult(None, rows=M, cols=D, drop_ld=D, p=0.5).to(dev)
        arg = dy.view(B, T, N, D).permute(0, 2, 1, 3).reshape(B, N, T * D).contiguous().bfloat16()
        kw, dy_eff = {"dy_seq_major": (T, N, _drop(0.5, D))}, dy * mult
    runs = []
    for _ in range(3):
        dx = torch.full((M, D), rc.NAN, device=dev)
        dg, db = ops.layernorm_bwd(arg, D, x, D, gamma, st, None, dx, M, D, **kw)
        runs.append((dx, dg.clone(), db.clone()))
    dx, dg, db = runs[0]
    agree = all(all(torch.equal(_bits(a), _bits(b)) for a, b in zip(r, runs[0])) for r in runs[1:])
    exact = dy_eff.to(torch.int64).sum(0)
    assert int(exact.abs().max()) < 2 ** 24
    ok_beta = torch.equal(db, exact.float())                   # a row lost in the grid-stride loop changes an integer
    ref, f32 = rc.ln_ref(x, gamma, dy_eff, torch.float64), rc.ln_ref(x, gamma, dy_eff, torch.float32)
    worst = 0.0
    for got, r64, r32, dims, name in ((dx, ref[0], f32[0], (-1,), "dx"), (dg, ref[1], f32[1], None, "dgamma")):
        need_gpu, need_f32 = rc.need_dev(got, r64, dims), rc.need_dev(r32, r64, dims)
        worst = max(worst, need_gpu / hi.bar_in_force(need_f32))
        assert hi.passes(need_gpu, need_f32), (M, D, variant, name, need_gpu, need_f32)
    _REC.append(("layernorm", f"M{M}_D{D}_{variant}", f"blocks={ops.layernorm_bwd_blocks(M, D)}", worst, "yes" if agree else "NO", "-"))
    assert ok_beta, (M, D, variant, "dbeta", float((db - exact.float()).abs().max()))
    assert agree, (M, D, variant)


@pytest.mark.parametrize("D", rc.LN_D)
def test_layernorm_partials_every_row_count(dev, D):
    """dbeta of an integer-valued dy is an exact sum (torch.equal against int64); dx and dgamma against float64 on the device
    with tests/hard_inputs.py's need / passes (K, FLOOR, BAR), the plain fp32 evaluation being torch's on the device."""
    from tecmollm import ops
    for M in rc.LN_M:
        assert ops.layernorm_bwd_blocks(M, D) == min((M + 3) // 4, 1024)
        _ln_check(ops, dev, M, D)


@pytest.mark.parametrize("variant", rc.LN_VARIANTS)
def test_layernorm_partials_other_gradient_forms(dev, variant):
    from tecmollm import ops
    M, D, _ = rc.LN_VARIANT_SHAPE
    _ln_check(ops, dev, M, D, variant)


def test_layernorm_refuses_other_widths(dev):
    from tecmollm import TecmError, ops
    for D in rc.LN_REFUSED_D:
        with pytest.raises(TecmError):
            ops.layernorm_bwd_blocks(5, D)


# ------------------------------------------------------------------------------------------------ GroupNorm partials
def _gn_check(ops, dev, kernel, B, N, monkeypatch):
    L, Cout, all16, split, path = rc.GN_KERNELS[kernel]
    monkeypatch.delenv("TECM_GN_BWD_WPS", raising=False)
    if split is None:
        monkeypatch.delenv("TECM_GN_BWD_SPLIT", raising=False)
    else:
        monkeypatch.setenv("TECM_GN_BWD_SPLIT", split)
    io = (ops.GN_Y_BF16 | ops.GN_OUT_BF16 | ops.GN_DACT_BF16) if all16 else 0
    assert ops.gn_bwd_path(L, N, Cout, io) == path, (kernel, B, N)
    CT = 3 * Cout
    y, dact, gamma, beta = rc.gn_case_inputs(kernel, B, N, dev)
    dt = torch.bfloat16 if all16 else torch.float32
    yk, dk = y.to(dt), dact.to(dt)
    st = torch.full((B * N, 3, 2), rc.NAN, device=dev)
    ops.groupnorm_gelu_fwd(yk, gamma, beta, torch.empty(B, L, N, CT, device=dev, dtype=dt), st, B, L, N, Cout)
    runs = []
    for _ in range(2 if B * N > 4096 else 3):
        dy = torch.full((B, L, N, CT), rc.NAN, device=dev, dtype=dt)
        runs.append((dy,) + tuple(t.clone() for t in ops.groupnorm_gelu_bwd(dk, 1, yk, gamma, beta, st, dy, B, L, N, Cout)))
    agree = all(all(torch.equal(_bits(a), _bits(b)) for a, b in zip(r, runs[0])) for r in runs[1:])
    dy, dg, db, dysum = runs[0]
    del runs
    gy, gg, gb, gs = rc.gn_ref(y, dact, gamma, beta, Cout)
    errs = {"dy": _rel(dy, gy) / (TOL_BF16 if all16 else TOL), "dgamma": _rel(dg, gg) / TOL, "dbeta": _rel(db, gb) / TOL,
            "dysum": _rel(dysum, gs) / TOL}
    worst = max(errs.values())
    _REC.append(("groupnorm", f"{kernel}_B{B}_N{N}", path, worst, "yes" if agree else "NO", "-"))
    assert worst < 1.0, (kernel, B, N, errs)
    assert agree, (kernel, B, N)


@pytest.mark.parametrize("kernel", list(rc.GN_KERNELS))
def test_groupnorm_partials_every_sequence_count(dev, monkeypatch, kernel):
    """dgamma, dbeta, the column sums of dy and dy against float64 GroupNorm(1) + GELU on the device, at S = B * N either side
    of one block's four sequences and of the 1024-block cap, where a block visits a second round of sequences."""
    from tecmollm import ops
    for S, (B, N) in rc.GN_S.items():
        _gn_check(ops, dev, kernel, B, N, monkeypatch)
    for B, N in rc.GN_SPLIT_ITEMS.get(kernel, ()):
        _gn_check(ops, dev, kernel, B, N, monkeypatch)


# ------------------------------------------------------------------------------------------------ Huber
def _huber_compare(loss, dpred, r, n, gs, tag):
    want_loss, want_d = rc.huber_exact_ref(r, n, gs)
    ulps = rc.ulps32(loss.item(), want_loss)
    _REC.append(("huber", tag, f"blocks={min((n + 255) // 256, rc.HUBER_BLOCK_CAP)}", ulps / 2, "-", "-"))
    assert torch.equal(dpred, want_d.to(dpred.device)), (tag, "dpred")
    assert ulps <= 2.0, (tag, "loss", loss.item(), want_loss, ulps)


def test_huber_flat_exact_either_side_of_the_block_cap(dev):
    from tecmollm import ops
    for k, n in enumerate(rc.HUBER_N):
        gs = rc.HUBER_GRAD_SCALES[k % 3]
        pred, target, r = rc.huber_exact_inputs((n,), 0)
        loss, dpred = ops.huber_fwd_bwd(pred.to(dev), target.to(dev), 1.0, gs)
        _huber_compare(loss, dpred, r, n, gs, f"flat_n{n}")
        loss2, none = ops.huber_fwd_bwd(pred.to(dev), target.to(dev), 1.0, gs, want_grad=False)
        assert none is None and torch.equal(loss, loss2)


def test_huber_strided_exact_on_the_permuted_prediction_view(dev):
    from tecmollm import ops
    for k, (B, H, N) in enumerate(rc.HUBER_STRIDED):
        gs = rc.HUBER_GRAD_SCALES[k % 3]
        pred_l, target_l, r = rc.huber_exact_inputs((B, H, N, 1), 1)
        storage = pred_l.squeeze(-1).permute(0, 2, 1).contiguous().to(dev)               # (B, N, L_out), as the head leaves it
        pred = storage.permute(0, 2, 1).unsqueeze(-1)
        wide = torch.full((B, H + 1, N + 2, 1), rc.NAN, device=dev)                      # the target in a layout of its own
        target = wide[:, :H, 1:N + 1]
        target.copy_(target_l)
        loss, dpred = ops.huber_fwd_bwd_strided(pred, target, 1.0, gs)
        assert dpred.stride() == pred.stride()
        _huber_compare(loss, dpred, r, B * H * N, gs, f"strided_B{B}_H{H}_N{N}")
        flat = ops.huber_fwd_bwd(pred.contiguous(), target.contiguous(), 1.0, gs)
        assert torch.equal(flat[1], dpred.contiguous())


# ------------------------------------------------------------------------------------------------ clip norm + AdamW
def _adamw_step(dev, p, g, m, v, *, zero_grad, max_norm, weight_decay, step, grad_scale):
    from tecmollm._lib import TecmAdamW, check, lib
    t = [x.clone().to(dev) for x in (p, g, m, v)]
    partials = torch.full((rc.NORM_BLOCKS,), rc.NAN, device=dev, dtype=torch.float64)
    norm = torch.full((1,), rc.SENTINEL, device=dev)
    a = TecmAdamW(n=p.numel(), param=t[0].data_ptr(), grad=t[1].data_ptr(), exp_avg=t[2].data_ptr(), exp_avg_sq=t[3].data_ptr(),
                  partials=partials.data_ptr(), total_norm_out=norm.data_ptr(), weight_decay=weight_decay, max_norm=max_norm,
                  grad_scale=grad_scale, step=step, zero_grad=zero_grad, **rc.ADAMW_HYPER)
    check(lib().tecm_adamw_clip_step(C.byref(a), _stream()), "tecm_adamw_clip_step")
    return norm, t


def test_clip_norm_is_exact_and_adamw_matches_float64(dev):
    for k, n in enumerate(rc.ADAMW_N):
        zg, max_norm, wd, step, gs = rc.ADAMW_OPTS[k % len(rc.ADAMW_OPTS)]
        p, g, m, v = rc.adamw_inputs(n)
        norm, (p1, g1, m1, v1) = _adamw_step(dev, p, g, m, v, zero_grad=zg, max_norm=max_norm, weight_decay=wd, step=step, grad_scale=gs)
        want = rc.exact_norm(g, gs)
        ulps = abs(norm.item() - want) / float(np.spacing(np.float32(want))) if want else abs(norm.item())
        _, pr, mr, vr = rc.adamw_ref(p.to(dev), g.to(dev), m.to(dev), v.to(dev), weight_decay=wd, max_norm=max_norm, grad_scale=gs,
                                     step=step, **rc.ADAMW_HYPER)
        worst = max(float(((a.double() - b).abs() / (rc.ADAMW_ATOL + rc.ADAMW_RTOL * b.abs())).max()) for a, b in ((p1, pr), (m1, mr), (v1, vr)))
        _REC.append(("adamw", f"n{n}_zg{zg}_clip{max_norm:g}_wd{wd:g}_step{step}", f"norm_blocks={min(max((n // 4 + 255) // 256, 1), rc.NORM_BLOCKS)}",
                     max(worst, ulps), "-", "-"))
        assert ulps <= 1.0, (n, "total_norm", norm.item(), want, ulps)
        assert worst <= 1.0, (n, "p, m, v", worst)
        assert torch.equal(g1, torch.zeros_like(g1) if zg else g.to(dev)), (n, "zero_grad", zg)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_gradient_does_what_torchs_clip_and_adamw_do(dev, bad):
    """clip_grad_norm_(1.0) + AdamW.step() on the CPU: a NaN norm makes the clip coefficient NaN (clamp(max=1) keeps it) and
    every parameter NaN; an infinite norm makes it 0, which poisons the infinite element alone."""
    n = 1027
    p, g, m, v = rc.adamw_inputs(n)
    g[7] = bad
    for zg, wd, step in ((1, 0.01, 1), (0, 0.0, 1000)):
        norm, (p1, g1, m1, v1) = _adamw_step(dev, p, g, m, v, zero_grad=zg, max_norm=1.0, weight_decay=wd, step=step, grad_scale=1.0)
        q = torch.nn.Parameter(p.clone())
        q.grad = g.clone()
        opt = torch.optim.AdamW([q], lr=rc.ADAMW_HYPER["lr"], betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        tn = torch.nn.utils.clip_grad_norm_([q], 1.0)
        opt.step()
        assert (math.isnan(norm.item()) and math.isnan(float(tn))) or norm.item() == float(tn) == math.inf, (bad, norm.item(), float(tn))
        for got, want, name in ((p1, q.detach(), "p"), (m1, opt.state[q]["exp_avg"], "m"), (v1, opt.state[q]["exp_avg_sq"], "v")):
            got = got.cpu()
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (bad, name, int(torch.isnan(got).sum()), int(torch.isnan(want).sum()))
            torch.testing.assert_close(got, want, rtol=rc.ADAMW_RTOL, atol=rc.ADAMW_ATOL, equal_nan=True)
        assert torch.equal(g1.cpu(), torch.zeros(n)) if zg else True


# ------------------------------------------------------------------------------------------------ checksum
def _tail(dev, param, world, rank):
    from tecmollm._lib import check, lib
    tail = torch.full((2 * world + 3,), rc.SENTINEL, device=dev)
    ws = torch.full((rc.CSUM_BLOCKS,), rc.NAN, device=dev, dtype=torch.float64)
    check(lib().tecm_checksum_tail(param.data_ptr(), param.numel(), tail.data_ptr(), world, rank, ws.data_ptr(), _stream()),
          "tecm_checksum_tail")
    return tail


def test_checksum_pair_is_the_exact_sum_in_its_own_slots(dev):
    for n in rc.CSUM_N:
        param = torch.randint(0, 2 ** 21, (n,), generator=rc.gen("csum", n)).float().to(dev)       # sums pass 2^24: lo is in use
        exact = int(param.to(torch.int64).sum())
        for world in rc.CSUM_WORLDS:
            for rank in range(world):
                tail = _tail(dev, param, world, rank).cpu().double()
                assert tail[2 * rank].item() + tail[2 * rank + 1].item() == exact, (n, world, rank)
                others = torch.cat([tail[:2 * rank], tail[2 * rank + 2:2 * world]])
                assert bool((others == 0).all()) and bool((tail[2 * world:] == rc.SENTINEL).all()), (n, world, rank)
        _REC.append(("checksum", f"n{n}", f"blocks={min((n + 255) // 256, rc.CSUM_BLOCKS)}", 0.0, "-", "-"))
    assert exact > 2 ** 24 and tail[2 * rank + 1].item() != 0


def test_checksum_verify_flags_one_differing_rank_and_a_nan(dev):
    from tecmollm._lib import check, lib
    bit = 4

    def verify(tail, world):
        err = torch.ones(1, device=dev, dtype=torch.int32)                               # another bit, already set, stays
        check(lib().tecm_checksum_verify(tail.data_ptr(), world, err.data_ptr(), bit, _stream()), "tecm_checksum_verify")
        return err.item()

    param = torch.randint(0, 2 ** 21, (65537,), generator=rc.gen("csum-verify")).float().to(dev)
    for world in rc.CSUM_WORLDS:
        summed = sum(_tail(dev, param, world, r)[:2 * world] for r in range(world))      # what the SUM all-reduce leaves
        assert verify(summed, world) == 1
        for r in range(1, world):
            for slot in (2 * r, 2 * r + 1):
                off = summed.clone()
                off[slot] = off[slot] + 1.0 if slot % 2 else off[slot] * 1.5
                assert off[slot] != summed[slot] and verify(off, world) == 1 | bit, (world, r, slot)
            nan = summed.clone()
            nan[2 * r] = rc.NAN
            assert verify(nan, world) == 1 | bit, (world, r)
        nan = summed.clone()
        nan[0] = rc.NAN                                                                  # NaN != NaN: rank 0's own slot is flagged too
        assert verify(nan, world) == 1 | bit
