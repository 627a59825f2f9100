"""CPU tests that keep the GEMM shape-boundary matrix (tests/gemm_shape_cases.py, tests/test_gpu_gemm_shapes.py) honest: the
table holds every edge with its neighbours and names a kernel for every case, correct fp32 arithmetic passes every case far
inside the bars, one k-term of one element is worth more than that element's bar on every shape, results that are wrong
the way a ragged-tile bug makes them wrong fail the comparison, and the window cases' reference is torch's conv1d."""
import pytest
import torch

from tests import gemm_epilogue_cases as T
from tests import gemm_epilogue_ref as R
from tests import gemm_shape_cases as S

FAMILIES = [f.name for f in S.SHAPE_FAMILIES]


# ------------------------------------------------------------------------------------------------ table integrity
@pytest.mark.parametrize("name", FAMILIES)
def test_every_edge_has_its_neighbours_and_every_case_a_kernel(name):
    fam = S.SHAPE_FAMILY[name]
    table = S.shapes(fam)
    assert 0 < len(table) <= S.CASE_BUDGET, len(table)
    assert len(set(table)) == len(table)
    refused = {(s.M, s.N, s.K) for s in fam.refused}
    have = {(s.M, s.N, s.K) for s in table if s == S.shape(s.M, s.N, s.K)}
    for i, axis in enumerate("MNK"):
        for e in fam.edges.get(axis, ()):
            for v in (e - fam.step[i], e, e + fam.step[i]):
                mnk = list(fam.base)
                mnk[i] = v
                assert v <= 0 or tuple(mnk) in have or tuple(mnk) in refused, (axis, e, v)
    if fam.corner:
        for dm in (-1, 0, 1):
            for dn in (-1, 0, 1):
                for dk in (-1, 0, 1):
                    c = (fam.corner[0] + dm * fam.cstep[0], fam.corner[1] + dn * fam.cstep[1], fam.corner[2] + dk * fam.cstep[2])
                    assert c in have, c
    kernels = set()
    for s in table:
        assert S.refusal(fam, s) is None, s                          # what the contract refuses is listed as refused
        assert S.probes_of(fam, s)[0] == "bare"
        for p in S.probes_of(fam, s):
            assert T.refusal(S.PROBES[p]) is None
            k = S.expected_kernel(fam, s, p, S.inputs_for(fam, s).ldc_of(S.PROBES[p]))
            assert isinstance(k, str) and k.startswith("gemm_"), (s, p)
            kernels.add(k)
    for s in fam.refused:
        assert S.refusal(fam, s), s
    # the base shape runs the family's own kernel
    own = {"bf16_dma1": "gemm_bf16_dma_kernel", "bf16_dma2": "gemm_bf16_dma2_kernel", "bf16_dma5": "gemm_bf16_dma5_kernel",
           "bf16_dma8": "gemm_bf16_dma5w_kernel", "bf16_p8_128": "gemm_bf16_p8_kernel<128>",
           "bf16_p8_112": "gemm_bf16_p8_kernel<112>", "bf16_p8_96": "gemm_bf16_p8_kernel<96>", "bf16x3": "gemm_x3_kernel<2,32>",
           "bf16x6": "gemm_x3_kernel<3,16>", "f32_km_kn_m64": "gemm_kernel<1,1,4,4,128,false,false,64>",
           "default_dispatch": "gemm_bf16_dma2_kernel"}
    base = S.shape(*fam.base)
    if name in own:
        assert S.expected_kernel(fam, base, "bare", S.inputs_for(fam, base).ldc) == own[name]
    if name == "bf16_tn":
        assert "gemm_bf16_tn_kernel" in kernels and "gemm_bf16_kernel<1,1,true,false>" in kernels
        for m, n in S._TN_GEO:
            for k in (4096, 4104, 4127):
                assert S.expected_kernel(fam, S.shape(m, n, k), "split", n + 4) == "gemm_bf16_tn_kernel"
            assert S.real_splits(4127, S.SPLIT_ASKED, 32) == 3
        for m, n, k in ((192, 256, 4095), (200, 256, 4104)):
            assert S.shape(m, n, k) in table and S.expected_kernel(fam, S.shape(m, n, k), "split", n + 4) != "gemm_bf16_tn_kernel"
    if name == "default_dispatch":                                   # every kernel the library chooses by itself
        assert kernels >= {"gemm_bf16_kernel<0,0,false,false>", "gemm_bf16_dma2_kernel", "gemm_bf16_dma5_kernel",
                           "gemm_bf16_dma_kernel", "gemm_bf16_p8_kernel<112>"}, kernels


def test_alignment_cases_state_what_pick_vec_and_the_vec4_rule_select():
    reached = set()
    for fam in S.SHAPE_FAMILIES:
        for s in fam.align:
            inst = S.loader_instance(fam, s)
            assert s.inst == f"({inst[0]},{inst[1]})", (fam.name, s)
            ldc = S.inputs_for(fam, s).ldc
            assert s.epi == ("vec4" if S.epilogue_vec4(fam, s, "bare", ldc) else "scalar"), (fam.name, s)
            assert f",{inst[0]},{inst[1]}," in S.expected_kernel(fam, s, "bare", ldc)
            if s.M % 128 and s.N % 128 and s.K % 32:                 # ragged in M, N and K
                reached.add((inst, s.epi))
    for inst in ((4, 4), (2, 1), (4, 2), (1, 1)):
        assert (inst, "vec4") in reached and (inst, "scalar") in reached, inst
    offs = {(s.a_off, s.b_off, s.c_off) for f in S.SHAPE_FAMILIES for s in f.align}
    assert {o[0] for o in offs} >= {0, 1, 2} and {o[1] for o in offs} >= {0, 1, 2} and {o[2] for o in offs} >= {1, 2, 4}
    fam = S.SHAPE_FAMILY["f32_mk_nk"]
    assert {S.lds(fam, s)[0] - s.K for s in fam.align} >= {0, 1, 2, 4}


def test_split_sweep_reaches_every_reducer_with_real_counts():
    for name, (d, bk) in S.SPLIT_FAMILIES.items():
        fam = S.SHAPE_FAMILY[name]
        cases = S.split_cases(name)
        assert {c.real for c in cases if c.asked == c.real} >= set(S.SPLIT_COUNTS)
        assert {S.reducer(c.real) for c in cases} >= {4, 8, 16}
        assert any(c.asked > c.real for c in cases)
        assert any(c.K % bk and c.real == c.asked and c.K > (c.real - 1) * bk for c in cases)     # a last split of one short K-tile
        for c in cases:
            s = S.split_shape(c)
            assert S.refusal(fam, s) is None
            assert S.kernel_bk(S.expected_kernel(fam, s, "split", S.inputs_for(fam, s).ldc)) == bk, (name, c)
            assert 1 <= c.real <= c.asked and (c.real - 1) * S._up((c.K + c.asked - 1) // c.asked, bk) < c.K
    assert S.real_splits(40, 3, 64) == 1                                  # the note of tests/test_gpu_gemm_epilogue.py


# ------------------------------------------------------------------------------------------------ room under the bars
def _fp32_result(inp, c, c_off):
    """The contract evaluated in fp32 (product included) into a pre-filled buffer, as a kernel would leave it."""
    prefill = inp.prefill(c, c_off)
    got, pre, _ = R.epilogue_ref(inp.A @ inp.B.t(), prefill[c_off:].float(), inp.ldc_of(c), dtype=torch.float32,
                                 **inp.ref_kwargs(c))
    got = torch.cat([prefill[:c_off].float(), got])
    got_pre = None
    if c.pre:
        got_pre = torch.full((inp.fam.M, inp.ld), float("nan"))
        got_pre[:, :inp.fam.N] = pre
    return (got.bfloat16() if c.c16 else got), got_pre, prefill


def _all_inputs():
    seen = {}
    for fam in S.SHAPE_FAMILIES:
        for s in S.shapes(fam):
            key = (s.M, s.N, s.K, fam.prec == 1, s.ldc, s.c_off)
            seen.setdefault(key, set()).update(S.probes_of(fam, s))
    for name in S.SPLIT_FAMILIES:
        for sc in S.split_cases(name):
            seen.setdefault((S.SPLIT_MN[0], S.SPLIT_MN[1], sc.K, S.SHAPE_FAMILY[name].prec == 1, None, S.C_OFF), set()).update(S.SPLIT_PROBES)
    return seen


def test_fp32_arithmetic_passes_every_case_and_one_term_outweighs_the_bar():
    """Every accepted (shape, probe) evaluated in fp32 on the CPU sits below 0.1 of the element bar, and on every shape one
    k-term of one element is worth at least 1.5 element bars (measured: fp32 <= 0.0033; the margin's lower bound 1.64 at
    K = 4127, the largest K of the table)."""
    worst, least, failures, n = 0.0, float("inf"), [], 0
    for (M, N, K, rounded, ldc, c_off), probes in _all_inputs().items():
        inp = S.inputs_of(M, N, K, rounded, ldc)
        margin = S.term_margin(inp)
        least = min(least, margin)
        if not margin >= 1.5:
            failures.append(f"{M}x{N}x{K}: one term is only {margin:.3g} bars")
        for p in sorted(probes):
            c = S.PROBES[p]
            got, got_pre, prefill = _fp32_result(inp, c, c_off)
            fails, err = S.check_shape(inp, c, got, got_pre, prefill, c_off)
            n += 1
            worst = max(worst, err or 0.0)
            failures += [f"{M}x{N}x{K} {p}: {f}" for f in fails]
    print(f"\n{n} cases, largest fp32 elem_err {worst:.3g}, least term margin {least:.3g}")
    assert not failures, failures[:20]
    assert worst < 0.1 and n > 1000


# ------------------------------------------------------------------------------------------------ mutations
def _mutants(inp, K):
    """(what, function on the (M, N) block of a correct bare result): the ways a ragged-tile bug is wrong."""
    A, B, M, N = inp.A.double(), inp.B.double(), inp.fam.M, inp.fam.N
    a = T.ALPHA
    out = [("one k-term dropped at the last corner", lambda C: C[M - 1, N - 1].sub_(a * A[M - 1, K - 1] * B[N - 1, K - 1])),
           ("one k-term dropped at the first corner", lambda C: C[0, 0].sub_(a * A[0, 0] * B[0, 0])),
           ("one k-term doubled", lambda C: C[M // 2, N // 2].add_(a * A[M // 2, K // 2] * B[N // 2, K // 2])),
           ("last row with K - 1 terms", lambda C: C[M - 1].sub_(a * A[M - 1, K - 1] * B[:, K - 1])),
           ("last column with K - 1 terms", lambda C: C[:, N - 1].sub_(a * A[:, K - 1] * B[N - 1, K - 1]))]
    if K > 1:
        lo, hi = (K // 3, 2 * (K // 3)) if K >= 3 else (1, 2)
        out.append(("one slab of a split left out", lambda C: C.sub_(a * A[:, lo:hi] @ B[:, lo:hi].t())))
    for seam in (64, 128, 256):
        if M > seam:
            def swap(C, r=seam):
                C[[r - 1, r]] = C[[r, r - 1]]
            out.append((f"rows {seam - 1} and {seam} swapped", swap))
    return out


@pytest.mark.parametrize("name", FAMILIES)
def test_results_wrong_like_a_ragged_tile_bug_fail_the_comparison(name):
    fam = S.SHAPE_FAMILY[name]
    table = S.shapes(fam)
    picks = {S.shape(*fam.base), max(table, key=lambda s: s.K), max(table, key=lambda s: s.M * s.N)}
    c = S.PROBES["bare"]
    for s in picks:
        inp = S.inputs_for(fam, s)
        ldc, off = inp.ldc_of(c), s.c_off
        good, _, prefill = _fp32_result(inp, c, off)
        assert S.check_shape(inp, c, good, None, prefill, off)[0] == []
        rows = torch.arange(s.M)[:, None] * ldc + torch.arange(s.N)[None, :] + off
        for what, mutate in _mutants(inp, s.K):
            bad = good.clone()
            block = bad[rows].double()
            mutate(block)
            bad[rows] = block.float()
            assert S.check_shape(inp, c, bad, None, prefill, off)[0], (s, what)
        if s.M > 1:                                                  # a pad column written (last row has none: exact size)
            bad = good.clone()
            bad[off + s.N] = 0.0
            assert "wrote outside its elements" in S.check_shape(inp, c, bad, None, prefill, off)[0], s
        if off:
            bad = good.clone()
            bad[off - 1] = 0.0
            assert "wrote in front of c_off" in S.check_shape(inp, c, bad, None, prefill, off)[0], s


# ------------------------------------------------------------------------------------------------ window view of A
def test_window_view_reference_is_conv1d():
    """The view of x written out row by row, times the weight as [n][tap Cw + c], is torch's conv1d in fp64; every case
    names a kernel or is refused for a reason; M sits either side of 128 and 256; one term outweighs the bar."""
    assert {w.B * w.Lout * w.nodes for w in S.WIN_CASES} >= {127, 128, 129, 255, 256, 257}
    assert {(w.taps, w.stride, w.Cw) for w in S.WIN_CASES} >= {(t, s, c) for t in (3, 7) for s in (1, 2) for c in (4, 6, 7, 24)}
    for w in S.WIN_CASES:
        for rounded in (False, True):
            inp = S.win_inputs(w, rounded)
            torch.testing.assert_close(inp.A.double() @ inp.B.double().t(), inp.P, rtol=1e-12, atol=1e-12)
            assert S.term_margin(inp) >= 1.5, w
            got, _, prefill = _fp32_result(inp, S.PROBES["bare"], S.C_OFF)
            fails, err = S.check_shape(inp, S.PROBES["bare"], got, None, prefill, S.C_OFF)
            assert not fails and err < 0.1, (w, fails, err)
        nodes, Lin, Lout, stride, taps, Cw, pad = S.win_geometry(w)
        assert pad == (taps - 1) // 2 and inp.x.shape == (w.B * Lin * nodes, Cw)
    names = {name: {S.win_expected(name, w) for w in S.WIN_CASES} for name in S.WIN_FAMILIES}
    assert names["f32_mk_nk"] == {f"gemm_kernel<0,0,{i},128,{f},128>" for i, f in (("4,4", "true,false"), ("2,1", "true,true"),
                                                                                 ("1,1", "true,true"))}
    assert names["bf16_reg_f32ops"] == {"gemm_bf16_kernel<0,0,true,false>", "gemm_kernel<0,0,2,1,128,true,true,128>",
                                        "gemm_kernel<0,0,1,1,128,true,true,128>"}
    assert names["bf16_res_a_mk_nk"] == {"gemm_bf16_kernel<0,0,true,false>", None}


def test_rows_factor_for_any_m():
    assert T.factor_rows(258) == (2, 3, 43) and T.factor_rows(64) == (2, 2, 16)        # what the epilogue matrix was wired to
    for M in (1, 2, 3, 127, 128, 255, 257, 300, 513):
        b, p, n = T.factor_rows(M)
        assert b * p * n == M and min(b, p, n) >= 1
