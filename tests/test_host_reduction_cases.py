"""The case tables of tests/reduction_cases.py without a GPU: every column-sum case gets the route it names from
tecm_colsum_path (the plan function the launchers route by, csrc/colsum.hip: colsum_plan), the tables reach every route and
both sides of every launcher edge, the references agree with torch's own, and a correct result altered the way a bug would
alter it fails the comparison of its case.  A launcher threshold that moves fails here instead of silently shrinking what
tests/test_gpu_reductions.py covers."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import hard_inputs as hi
from tests import reduction_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tec-mollm_amd", "tecmollm", "libtecmollm_hip.so")


@pytest.fixture(scope="module")
def ops():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    from tecmollm import ops
    return ops


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("TECM_COLSUM_MINROWS", raising=False)


def _path(ops, c):
    return ops.colsum_path(c.ld, c.outer, c.inner, c.nseg, c.C, 4 * (c.off % 4), 0)


def test_the_query_is_declared_bound_and_exported(ops):
    from tecmollm import _lib
    header = open(os.path.join(ROOT, "include", "tecmollm.h")).read()
    assert re.search(r"const char\* tecm_colsum_path\(int64_t ld, int64_t outer, int64_t inner, int32_t nseg, int32_t C,\s*"
                     r"int32_t in_misalign_bytes,\s*int32_t nbuf\);", header)
    assert "tecm_colsum_path" in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "tecm_colsum_path")
    # an additive entry point: the version stays
    assert _lib.ABI_VERSION == 21 == int(re.search(r"#define\s+TECM_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.lib().tecm_abi_version()


def test_every_column_sum_case_gets_the_route_it_names(ops):
    names = [c.name for c in rc.COLSUM]
    assert len(set(names)) == len(names)
    for c in rc.COLSUM:
        assert _path(ops, c) == c.route, c.name
        assert (c.rb - 1) * c.chunk < c.total <= c.rb * c.chunk, c.name          # the chunks cover the rows, none is empty
        assert c.rows * c.ld * 4 <= 100e6, c.name
    for t in rc.TWINS:
        assert ops.colsum_path(t.ld, t.outer, t.inner, t.nseg, t.C).startswith("v4 "), t.name
    for C, ld, _ in rc.TWIN_REFUSED:
        assert ops.colsum_path(ld, 37, 5, 3, C).startswith("scalar "), (C, ld)


def test_every_batch_case_gets_the_route_it_names(ops):
    for b in rc.BATCH:
        assert ops.colsum_path(b.C, b.rows, 1, 1, b.C, b.best_misalign, b.nbuf) == b.route, b.name
        assert b.rows * b.C * 4 <= 100e6 and b.nbuf * b.rows * b.C * 4 <= 250e6, b.name
        if b.route.startswith("each"):                  # one by one: a misaligned matrix among them takes the scalar stage
            assert ops.colsum_path(b.C, b.rows, 1, 1, b.C, 0, 0) == b.route[len("each "):]
            if b.misaligned:
                assert ops.colsum_path(b.C, b.rows, 1, 1, b.C, 4, 0).startswith("scalar ")
        else:                                           # its own launches: the blocks and chunks of tecm_colsum's scalar stage
            want = ops.colsum_path(b.C + 1, b.rows, 1, 1, b.C, 0, 0).replace("scalar", "batch")
            assert b.route == f"{want} launches={(b.nbuf + 31) // 32}", b.name


def test_the_tables_reach_every_route_the_launchers_have(ops):
    got = {(c.stage1, c.waves) for c in rc.COLSUM} | {(b.route.split()[0], int(b.route.split("waves=")[1].split()[0])) for b in rc.BATCH}
    assert got == rc.COLSUM_ROUTES
    assert any(b.route.endswith("launches=2") for b in rc.BATCH) and any(b.route.endswith("launches=1") for b in rc.BATCH)
    # ... and the two routes no table reaches cannot be reached: the lane-per-column first stages leave at most 256 partial
    # rows, the 16-wave second stage needs more.  The same sweep holds every route to the workspace the header promises.
    seen = set()
    for C in (1, 3, 4, 63, 64, 65, 128, 252, 256, 257, 260, 1020, 1024, 1025, 1028, 1536, 2304, 4096):
        for nseg in (1, 2, 3, 4, 5, 16, 1024, 1025):
            for total in (1, 15, 16, 17, 255, 256, 257, 4080, 4081, 4095, 4096, 4097, 16383, 16384, 16385, 70000, 10 ** 7):
                for ld, mis in ((C, 0), (C + 1, 0), (C, 4)):
                    r = ops.colsum_path(ld, total, 1, nseg, C, mis, 0)
                    st, rb, chunk, waves = r.split()[0], *(int(x.split("=")[1]) for x in r.split()[1:])
                    seen.add((st, waves))
                    assert rb >= 1 and (rb - 1) * chunk < total <= rb * chunk, (C, nseg, total, r)
                    assert rb * nseg <= max(1024, nseg), (C, nseg, total, r)              # workspace: 1024 * nseg * C floats
                    assert (waves == 16) == ((C + 63) // 64 * nseg <= 4 and rb > 256), (C, nseg, total, r)
                    if nseg == 1 and ld >= C:
                        for nbuf in (1, 32, 33):
                            rbat = ops.colsum_path(ld, total, 1, 1, C, mis, nbuf)
                            seen.add((rbat.split()[0], int(rbat.split("waves=")[1].split()[0])))
                            if rbat.startswith("batch"):
                                assert int(rbat.split("rb=")[1].split()[0]) <= 256, rbat     # workspace: 256 * nbuf * C floats
    assert seen == rc.COLSUM_ROUTES and not (seen & rc.COLSUM_UNREACHABLE)


def test_every_edge_is_hit_on_both_sides():
    for name, pred in rc.COLSUM_EDGES.items():
        sides = {pred(c) for c in rc.COLSUM} - {None}
        assert sides == {True, False}, name
    for name, pred in rc.BATCH_EDGES.items():
        assert {bool(pred(b)) for b in rc.BATCH} == {True, False}, name
    # the float4 stage at its 1024 / nseg block clamp with a ragged last chunk
    assert any(c.stage1 == "v4" and c.rb * c.nseg > 1000 and c.total % c.chunk for c in rc.COLSUM)
    # the issue's axes, each one present
    have = lambda f: {f(c) for c in rc.COLSUM}
    assert {1, 3, 4, 60, 64, 68, 252, 256, 260, 1020, 1024, 1028, 1536, 2304} <= have(lambda c: c.C)
    assert {0, 4, 1} <= have(lambda c: c.ld - c.C) and {0, 1, 4} <= have(lambda c: c.off)
    assert {1, 15, 16, 17, 4095, 4096, 4097, 16383, 16384, 16385, 20000, 70000} <= have(lambda c: c.total)
    assert {(s, i) for s in (1, 3, 4, 5) for i in (1, 5, 211)} <= have(lambda c: (c.nseg, c.inner))
    assert {(1.0, 0), (0.25, 1), (-2.0, 0), (-2.0, 1)} <= have(lambda c: (c.scale, c.acc))
    assert {(p, s) for p in (0.0, 0.5) for s in (1.0, 0.25, -2.0)} <= have(lambda c: (c.p, c.scale))
    assert {1, 7, 32, 33} <= {b.nbuf for b in rc.BATCH} and {6, 768, 1028, 1536} <= {b.C for b in rc.BATCH}
    assert {1, 300, 4096, 5000} <= {b.rows for b in rc.BATCH}
    # the other tables straddle the caps they name
    assert {4 * 1024 - 1, 4 * 1024, 4 * 1024 + 1} <= set(rc.LN_M) and {4 * 1024 - 1, 4 * 1024, 4 * 1024 + 1} <= set(rc.GN_S)
    assert all(b * n == s for s, (b, n) in rc.GN_S.items())
    cap = 256 * rc.HUBER_BLOCK_CAP
    assert {255, 256, 257, cap - 1, cap, cap + 1} <= set(rc.HUBER_N) and max(b * h * n for b, h, n in rc.HUBER_STRIDED) > cap
    assert {1024 * rc.NORM_BLOCKS - 1, 1024 * rc.NORM_BLOCKS} <= set(rc.ADAMW_N) and max(rc.ADAMW_N) > 1024 * rc.ADAMW_BLOCK_CAP
    assert {n & 3 for n in rc.ADAMW_N} == {0, 1, 2, 3}
    assert {256 * rc.CSUM_BLOCKS - 1, 256 * rc.CSUM_BLOCKS, 256 * rc.CSUM_BLOCKS + 1} <= set(rc.CSUM_N)
    for kern, shapes in rc.GN_SPLIT_ITEMS.items():
        group = 10 if kern == "split64" else 5
        assert {n - group for _, n in shapes} == {-1, 0, 1}
        for b, n in shapes:
            items, blocks = rc.gn_items(kern, b, n)
            assert items > blocks >= 900, (kern, b, n)


def test_refusals_give_no_path(ops):
    assert ops.colsum_path(4, 0, 1, 1, 4) == "" and ops.colsum_path(4, 1, 0, 1, 4) == "" and ops.colsum_path(4, 1, 1, 0, 4) == ""
    assert ops.colsum_path(4, 1, 1, 1, 0) == "" and ops.colsum_path(4, 1, 1, 1, 4, 0, -1) == ""
    assert ops.colsum_path(4, 8, 2, 1, 4, 0, 3) == "" and ops.colsum_path(4, 8, 1, 2, 4, 0, 3) == ""      # a batch has no segments
    assert ops.colsum_path(3, 8, 1, 1, 4, 0, 3) == ""                                                       # ... and ld >= C


def test_exact_references_are_exact_and_an_altered_result_fails_its_case():
    """The EXACT family on the host: the int64 sums stay below 2^24 through mask, scale and accumulation, and every
    alteration that changes an integer changes the fp32 result the comparison (torch.equal) sees."""
    shown = {a: 0 for a in rc.ALTERATIONS}
    applicable = {a: 0 for a in rc.ALTERATIONS}
    for c in rc.COLSUM:
        buf = rc.colsum_buffer(c, "exact")
        vals = rc.colsum_values(buf, c)
        assert not torch.isnan(vals).any() and (c.ld == c.C or torch.isnan(buf[c.off:c.off + c.rows * c.ld].view(c.rows, c.ld)[:, c.C:]).all())
        mult = rc.colsum_mult(c)
        assert mult is None or set(mult.unique().tolist()) == {0.0, 2.0}
        out0 = rc.colsum_out0(c, "exact")
        m = rc.colsum_int_sums(vals, mult, c)
        sums = m.sum(1)
        ref = rc.colsum_ref_exact(vals, mult, c, out0)
        assert ref.dtype == torch.float32 and torch.equal(ref.double(), sums.double() * c.scale + (out0.double() if c.acc else 0))
        for name, alt in rc.colsum_alterations(m, c):
            applicable[name] += 1
            if not torch.equal(alt, sums):                   # (a dropped row of zeros in a one-column case alters nothing)
                shown[name] += 1
                assert not torch.equal(rc.colsum_finish_exact(alt, c, out0), ref), (c.name, name)
    for name in rc.ALTERATIONS:
        assert applicable[name] >= 20 and shown[name] >= 0.9 * applicable[name], (name, shown[name], applicable[name])


def test_the_real_bound_holds_for_fp32_sums_in_other_orders_and_catches_a_wrong_scale_or_mask():
    for c in [c for c in rc.COLSUM if c.name in ("C68", "C3", "rows4097_C64", "C70_nseg3_inner211", "mask_C68_ld72_dropld75")]:
        vals = rc.colsum_values(rc.colsum_buffer(c, "real"), c)
        mult, out0 = rc.colsum_mult(c), rc.colsum_out0(c, "real")
        ref, bound = rc.colsum_ref_real(vals, mult, c, out0)
        m = vals if mult is None else vals * mult.view(c.outer, c.nseg, c.inner, c.C)
        seq = m.permute(1, 0, 2, 3).reshape(c.nseg, c.total, c.C)
        for order in (seq, seq.flip(1)):                     # torch's pairwise fp32 sum and a plain running one
            run = torch.zeros(c.nseg, c.C)
            for r in range(c.total):
                run = run + order[:, r]
            for s in (order.sum(1), run):
                got = s * c.scale + (out0 if c.acc else 0)
                assert rc.real_ratio(got, ref, bound) <= 1.0, c.name
        wrong_scale = seq.sum(1) * (c.scale * 1.5) + (out0 if c.acc else 0)
        assert rc.real_ratio(wrong_scale, ref, bound) > 1.0, c.name
        if mult is not None:
            unmasked = vals.permute(1, 0, 2, 3).reshape(c.nseg, c.total, c.C).sum(1) * c.scale + (out0 if c.acc else 0)
            assert rc.real_ratio(unmasked, ref, bound) > 1.0, c.name
    assert rc.real_ratio(torch.tensor([float("nan")]), torch.zeros(1, dtype=torch.float64), torch.ones(1, dtype=torch.float64)) == math.inf
    assert float(rc.ulp32(torch.tensor([1.0, 3.0, 2.0 ** 24], dtype=torch.float64))[2]) == 2.0


def test_need_dev_is_hard_inputs_need():
    g = torch.Generator().manual_seed(5)
    ref = torch.randn(37, 64, generator=g, dtype=torch.float64)
    got = (ref + 1e-4 * torch.randn(37, 64, generator=g, dtype=torch.float64)).float()
    for dims in ((-1,), None, ()):
        assert rc.need_dev(got, ref, dims) == pytest.approx(hi.need(got, ref, dims), rel=1e-12)
    got[3, 5] = float("inf")
    assert rc.need_dev(got, ref, (-1,)) == math.inf


def test_layernorm_and_groupnorm_references_and_the_exact_dbeta():
    x, gamma, dy, _ = rc.ln_case_inputs(37, 260)
    dx, dg, db = rc.ln_ref(x, gamma, dy, torch.float64)
    cpu = hi.ln_cpu(x, gamma, torch.zeros(260), dy, torch.float64)
    assert torch.equal(dx, cpu[3]) and torch.equal(dg, cpu[4]) and torch.equal(db, cpu[5])
    exact = dy.to(torch.int64).sum(0)
    assert torch.equal(db, exact.double()) and int(exact.abs().max()) < 2 ** 24
    assert not torch.equal(dy[:-1].to(torch.int64).sum(0).float(), exact.float())       # a row lost in the grid-stride loop
    y, dact, gamma, beta = rc.gn_case_inputs("split64", 2, 3, "cpu")
    full = hi.gn_cpu(y, gamma, beta, 64, dact, torch.float64)
    gy, gg, gb, gs = rc.gn_ref(y, dact, gamma, beta, 64)
    for mine, torchs in zip((gy, gg, gb, gs), full[3:]):             # written out here, autograd there
        torch.testing.assert_close(mine, torchs, rtol=1e-11, atol=1e-13)
    assert torch.equal(y, y.bfloat16().float()) and torch.equal(dact, dact.bfloat16().float())


def test_huber_exact_family_is_exact_and_matches_torch():
    for n, gs in ((257, 0.125), (300001, 4.0)):
        pred, target, r = rc.huber_exact_inputs((n,), 0)
        assert torch.equal(pred - target, r) and float(r.abs().max()) <= 3.0
        loss, dpred = rc.huber_exact_ref(r, n, gs)
        pd = pred.double().requires_grad_(True)
        want = torch.nn.functional.huber_loss(pd, target.double(), delta=1.0)
        assert loss == pytest.approx(float(want.detach()), rel=1e-13)
        gw, = torch.autograd.grad(want, pd)
        torch.testing.assert_close(dpred.double(), gw * gs, rtol=2.0 ** -23, atol=0)
        a = r.abs()
        terms = torch.where(a <= 1, 0.5 * a * a, a - 0.5)
        assert torch.equal(terms * 32, (terms * 32).round()) and float(terms.double().sum()) < 2 ** 19        # exact in any order
        assert rc.ulps32(np.float32(loss), loss) <= 0.5 and rc.ulps32(np.float32(loss) * np.float32(1 + 2.0 ** -21), loss) > 2


def test_adamw_reference_is_torchs_and_an_unwritten_tail_fails():
    for n, (zg, max_norm, wd, step, gs) in zip((5, 1025), rc.ADAMW_OPTS[2:4]):
        p, g, m, v = rc.adamw_inputs(n)
        norm, p1, m1, v1 = rc.adamw_ref(p, g, m, v, weight_decay=wd, max_norm=max_norm, grad_scale=gs, step=step, **rc.ADAMW_HYPER)
        q = torch.nn.Parameter(p.double().clone())
        q.grad = g.double() * gs
        opt = torch.optim.AdamW([q], lr=rc.ADAMW_HYPER["lr"], betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
        tn = torch.nn.utils.clip_grad_norm_([q], max_norm) if max_norm > 0 else q.grad.norm()
        opt.step()
        assert norm == pytest.approx(float(tn), rel=1e-14)
        torch.testing.assert_close(p1, q.detach(), rtol=1e-13, atol=1e-15)
        torch.testing.assert_close(m1, opt.state[q]["exp_avg"], rtol=1e-13, atol=1e-15)
        torch.testing.assert_close(v1, opt.state[q]["exp_avg_sq"], rtol=1e-13, atol=1e-15)
        assert rc.exact_norm(g, gs) == pytest.approx(norm, rel=2.0 ** -23)
        tail = p1.float().clone()
        tail[n - (n & 3):] = p[n - (n & 3):]                 # the tail n & 3 skipped
        assert not torch.allclose(tail.double(), p1, rtol=rc.ADAMW_RTOL, atol=rc.ADAMW_ATOL)
        # a gradient left out of the norm: one fp32 ulp does not cover it
        short = rc.exact_norm(g[:-1], gs)
        assert g[-1] == 0 or abs(short - rc.exact_norm(g, gs)) > float(np.spacing(np.float32(rc.exact_norm(g, gs))))
