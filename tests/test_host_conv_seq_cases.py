"""CPU tests of tests/conv_seq_cases.py: the case lists of the sequence-tile conv kernels are pinned (counts, and every class of
tile plan present, judged by the library's own tecm_conv_{fwd,dx}_tile_steps); predicates and launchers refuse the same shapes
before any launch; the exact inputs are exact; the two comparisons notice every planted fault they are meant to notice."""
import ctypes as C

import pytest
import torch

from tests import conv_seq_cases as cs


def _count(cases):
    return sum(not c.f32 for c in cases), sum(c.f32 for c in cases)


def test_case_lists_are_pinned():
    """(bf16, fp32) cases per kernel: the one-axis sweeps and the seeded sample of 12 + 12; what the sweeps found refused."""
    assert _count(cs.FWD_SWEEP) == (59, 62) and _count(cs.FWD_SAMPLE) == (12, 12)
    assert _count(cs.DX_SWEEP) == (63, 57) and _count(cs.DX_SAMPLE) == (12, 12)
    assert _count(cs.DW_SWEEP) == (41, 41) and _count(cs.DW_SAMPLE) == (12, 12)
    for cases in cs.CASES.values():
        assert len(set(cases)) == len(cases) and all(c.B * c.N <= cs.MAX_SEQ for c in cases)
        assert {c.N % 4 for c in cases} == {0, 1, 2, 3} and {c.B for c in cases} == {1, 3, 2}
    # the fp32 forward's LDS limit: ld_in = 72 and 128 at Lc = 48; the fp32 d-input image of 256 and 448 channels past Lc = 8
    assert [(c.Lc, c.ld_in, c.f32) for c in cs.FWD_REFUSED] == [(48, 72, True), (48, 128, True)]
    assert [(c.Lc, c.ld_in, c.Cout, c.f32) for c in cs.DX_REFUSED] == [(48, 24, 256, True), (48, 24, 448, True),
                                                                      (24, 64, 256, True), (24, 64, 448, True)]
    assert cs.DW_REFUSED == []
    assert [cs.fwd_f32_max_ld(L) for L in cs.LCS] == [128, 128, 128, 96, 80, 64, 64, 64, 64, 64, 64]


def test_tile_steps_queries_report_the_plans_of_the_production_shapes():
    """tecm_conv_{fwd,dx}_tile_steps against the plans worked out by hand from conv_fwd_lds / conv_dx_plan; 0 where refused."""
    h = cs._h()
    assert h.tecm_conv_fwd_tile_steps(48, 64, 24, 0) == 48 and h.tecm_conv_fwd_tile_steps(104, 128, 64, 1) == 48
    assert h.tecm_conv_fwd_tile_steps(40, 64, 80, 1) == 40 and h.tecm_conv_fwd_tile_steps(40, 64, 88, 1) == 0
    assert h.tecm_conv_fwd_tile_steps(20, 64, 24, 0) == 0 and h.tecm_conv_fwd_tile_steps(48, 160, 24, 0) == 0
    dx = lambda Lc, Cout, ld, f32: cs.plan("dx", cs.Case(1, Lc, 4, ld, ld, Cout, f32))
    assert dx(24, 128, 64, True) == [24] and dx(48, 128, 64, True) == [16, 16, 16]
    assert dx(96, 64, 24, True) == [40, 40, 16] and dx(32, 192, 32, True) == [8, 8, 8, 8]
    assert dx(48, 64, 24, False) == [48] and dx(48, 128, 64, False) == [24, 24]
    assert h.tecm_conv_dx_tile_steps(16, 256, 64, 1) == 0 and h.tecm_conv_dx_tile_steps(16, 256, 64, 0) > 0
    assert h.tecm_conv_dx_tile_steps(8, 768, 24, 0) == 8 and h.tecm_conv_dx_tile_steps(8, 832, 24, 0) == 0


def test_every_class_of_tile_plan_is_in_the_sweeps():
    """A later change to a plan that drops a class from the lists fails here."""
    for f32 in (False, True):
        fwd = [(c, cs.plan("fwd", c)) for c in cs.FWD_CASES if c.f32 == f32]
        assert {p[0] // 8 for _, p in fwd if len(p) == 1} == {1, 2, 3, 4, 5, 6}             # the six k-loop instantiations
        assert {8, 24, 40} <= {p[-1] for _, p in fwd if len(p) > 1}                       # ragged last chunks
        assert {c.Cout for c, _ in fwd} == {32, 64, 96, 128}
        assert {(c.ld_in // 8) % 2 for c, _ in fwd} == {0, 1}
        assert {c.cin for c, _ in fwd} >= {1} and any(c.cin == c.ld_in - 7 for c, _ in fwd)
        dx = [(c, cs.plan("dx", c), (c.ld_in + 31) // 32) for c in cs.DX_CASES if c.f32 == f32]
        assert {nci for _, _, nci in dx} == {1, 2}
        assert {32, 36} <= {c.ld_in for c, _, _ in dx}                                    # either side of the NCI boundary
        assert any(len(p) == 1 for _, p, _ in dx)
        assert any(len(p) > 1 and len(set(p)) == 1 for _, p, _ in dx)                     # equal chunks
        assert any(len(p) > 1 and p[-1] < p[0] for _, p, _ in dx)                         # a ragged last chunk
        # a TC the LDS cap lowered: below both the accumulator limit (6 row tiles / NCI) and the sequence
        assert any(p[0] < min(8 * (6 // nci), c.Lc) for c, p, nci in dx)
        assert {c.Cout for c, _, _ in dx} >= ({64, 128, 192, 256} if f32 else {64, 128, 192, 256, 448, 512, 768})
        dw = [c for c in cs.DW_CASES if c.f32 == f32]
        assert {(c.ld_in, c.Cout) for c in dw} == set(cs.DW_PAIRS)
        assert {4, 20, 24, 28, 52, 100} <= {c.Lc for c in dw}                             # below, at, above 24; a rest of 4
        assert any(cs.plan("dw", c)[-1] == 4 and len(cs.plan("dw", c)) > 1 for c in dw)
    # the four d-input plans of the issue that names this file's purpose
    plans = {(c.Lc, c.Cout, c.ld_in): cs.plan("dx", c) for c in cs.DX_CASES if c.f32}
    assert plans[(24, 128, 64)] == [24] and plans[(48, 128, 64)] == [16, 16, 16] and plans[(96, 64, 24)] == [40, 40, 16]


def _aligned(buf):
    return (C.addressof(buf) + 15) & ~15


def test_predicate_and_launcher_agree_on_refusals():
    """Every refused shape of the grid: the predicate says 0, the tile-steps query says 0 and the launcher returns its error code
    before any launch (host memory as aligned non-null dummies: a launch would not survive them).  No admitted shape is called."""
    from tecmollm import _lib
    h = cs._h()
    live = (C.c_float * 64)()
    p = _aligned(live)
    grid = cs.refusal_grid()
    assert len(grid) >= 27
    kinds = {k for k, _ in grid}
    assert kinds == {"fwd", "dx", "dw"}
    for kind, c in grid:
        f32 = int(c.f32)
        if kind == "fwd":
            assert h.tecm_conv_fwd_supported(c.Lc, c.Cout, c.ld_in, f32) == 0, c
            assert h.tecm_conv_fwd_tile_steps(c.Lc, c.Cout, c.ld_in, f32) == 0
            d = _lib.TecmConvFwd(inp=p, wpack=p, bias=p, y=p, B=c.B, Lc=c.Lc, N=c.N, Cout=c.Cout, ld_in=c.ld_in, y_bf16=0,
                                 stats=None, eps=1e-5)
            rc = (h.tecm_conv_fwd_f32 if f32 else h.tecm_conv_fwd_bf16)(C.byref(d), None)
            assert rc == (-4 if c.Lc % 8 == 0 and c.Cout <= 128 and c.ld_in <= 128 else -1), (c, rc)    # TECM_E_LDS / TECM_E_ARG
        elif kind == "dx":
            assert h.tecm_conv_dx_supported(c.Lc, c.Cout, c.ld_in, f32) == 0, c
            assert h.tecm_conv_dx_tile_steps(c.Lc, c.Cout, c.ld_in, f32) == 0
            d = _lib.TecmConvDx(dy=p, wpack=p, dinp=p, B=c.B, Lc=c.Lc, N=c.N, Cout=c.Cout, ld_in=c.ld_in)
            rc = (h.tecm_conv_dx_f32 if f32 else h.tecm_conv_dx_bf16)(C.byref(d), None)
            assert rc == (-4 if c.Lc % 8 == 0 and c.ld_in <= 64 else -1), (c, rc)
        else:
            assert h.tecm_conv_dw_supported(c.Lc, c.Cout, c.ld_in) == 0, c
            d = _lib.TecmConvDw(inp=p, dy=p, workspace=p, dw3=p, dw5=p, dw7=p, B=c.B, Lc=c.Lc, N=c.N, Cout=c.Cout, Cin=c.cin,
                                ld_in=c.ld_in, num_blocks=4)
            rc = (h.tecm_conv_dw_f32 if f32 else h.tecm_conv_dw_bf16)(C.byref(d), None)
            assert rc == -1, (c, rc)
        assert len(h.tecm_last_error()) > 0
    # what the issue names, by name
    want = [("fwd", 72, 48, True), ("fwd", 88, 40, True), ("fwd", 104, 32, True)]
    for kind, ld, L, f32 in want:
        assert any(k == kind and c.ld_in == ld and c.Lc == L and c.f32 == f32 for k, c in grid), (kind, ld, L)
    assert any(k == "fwd" and c.Cout == 160 for k, c in grid) and any(k == "dx" and c.ld_in == 68 for k, c in grid)
    assert any(k == "dx" and (c.Lc, c.Cout, c.ld_in, c.f32) == (16, 256, 64, True) for k, c in grid)
    assert any(k == "dw" and (c.ld_in, c.Cout) not in cs.DW_PAIRS for k, c in grid)
    assert any(c.Lc % 8 for k, c in grid if k != "dw") and any(c.Lc % 4 for k, c in grid if k == "dw")


ALL = [(k, c) for k in ("fwd", "dx", "dw") for c in cs.CASES[k]]


def test_exact_inputs_are_exact_on_every_case():
    """The premise of the bit-for-bit comparisons: on the exact inputs the float32 and the float64 CPU convolutions agree bit for
    bit (every partial sum is representable, so no summation order can round), and all values are bf16 values."""
    for kind, c in ALL:
        d = cs.make_inputs(kind, c, exact=True)
        for t in [v for v in d.values() if torch.is_tensor(v)] + d.get("ws", []):
            assert torch.equal(t.bfloat16().float(), t)
        r64 = cs._flat(kind, cs.reference(kind, c, d))
        r32 = cs._flat(kind, cs.reference(kind, c, d, dtype=torch.float32))
        assert torch.equal(r32.double(), r64) and torch.equal(r64.float().double(), r64), (kind, c)
        assert float(r64.abs().max()) > 0


def _fault_cases(kind):
    """A chunked case with B > 1 and N > 1 per precision (every fault applies), and the first sweep case of each base."""
    out = []
    for f32 in (False, True):
        multi = [c for c in cs.CASES[kind] if c.f32 == f32 and c.B > 1 and c.N > 1 and len(cs.plan(kind, c)) > 1]
        assert multi, (kind, f32)
        out.append(multi[0])
    return out


@pytest.mark.parametrize("kind", ["fwd", "dx", "dw"])
def test_the_bars_notice_every_planted_fault(kind):
    """Each fault planted into the reference fails the exact comparison; all but a weight scaled by 1 + 2^-10 -- the size of the
    bf16 mode's own weight rounding, which no a-priori bar of the accumulation can see -- fail the random-input bar."""
    for c in _fault_cases(kind):
        tc = cs.plan(kind, c)[0]
        ex = cs.make_inputs(kind, c, exact=True)
        ref = cs.reference(kind, c, ex)
        rn = cs.make_inputs(kind, c, exact=False)
        rref = cs.reference(kind, c, rn)
        b = cs.bar(kind, c, rn, rref, out_bf16=False)
        assert cs.ratio(kind, rref, rref, b) == 0.0
        # the float32 CPU convolution of the same operands passes the bar it is derived for
        assert cs.ratio(kind, cs.reference(kind, c, rn, dtype=torch.float32), rref, b) <= 1.0
        for fault in cs.FAULTS:
            bad = cs.plant(kind, c, ex, fault, tc)
            assert not torch.equal(cs._flat(kind, bad), cs._flat(kind, ref)), (c, fault)
            r = cs.ratio(kind, cs.plant(kind, c, rn, fault, tc), rref, b)
            assert r > 1.0 or fault == "weight_scaled", (c, fault, r)
        if kind == "fwd" and not c.f32:                    # the bf16 y: the reference rounded once passes, a planted fault does not
            b16 = cs.bar(kind, c, rn, rref, out_bf16=True)
            assert cs.ratio(kind, rref.float().bfloat16(), rref, b16) <= 1.0
            assert cs.ratio(kind, cs.plant(kind, c, rn, "node_copy", tc).float().bfloat16(), rref, b16) > 1.0
