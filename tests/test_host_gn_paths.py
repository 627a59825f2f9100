"""The routing table of the GroupNorm(1)+GELU launchers (csrc/groupnorm.hip: gn_fwd_plan / gn_bwd_plan) without a GPU:
tecm_gn_fwd_path / tecm_gn_bwd_path name the kernel a call with aligned tensors launches, from the plan functions the
launchers route by.  The rows are literals read off the launchers' if-chains as they stood before the plan functions
existed (quads = L * 3*Cout/4 in whole rounds of 256 / 512 / 128 lanes with at most 9 / 9 / 18 per lane; octs =
L * 3*Cout/8 <= 1152 / 2304), and tecm_gn_reg_supported / tecm_gn_y16_supported are checked against the same paths."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tec-mollm_amd", "tecmollm", "libtecmollm_hip.so")

Y16, OUT16, DACT16, GIVEN = 1, 2, 4, 8          # TECM_GN_Y_BF16, _OUT_BF16, _DACT_BF16, _STATS_GIVEN
ALL16 = Y16 | OUT16 | DACT16

# (L, Cout) -> forward kernel with fp32 tensors, act_stride 1; `{io}` is the IO16 template argument of the register kernels
FWD = [(48, 64, "gn_gelu_fwd_reg<1,4,9,{io}>"), (24, 128, "gn_gelu_fwd_reg<2,4,9,{io}>"), (12, 256, "gn_gelu_fwd_reg<4,4,9,{io}>"),
       (96, 64, "gn_gelu_fwd_reg<1,8,9,{io}>"), (48, 128, "gn_gelu_fwd_reg<2,8,9,{io}>"),
       (24, 64, "gn_gelu_fwd_reg<1,2,18,{io}>"), (12, 128, "gn_gelu_fwd_reg<2,2,18,{io}>"), (6, 256, "gn_gelu_fwd_reg<4,2,18,{io}>"),
       (40, 64, "gn_gelu_fwd_reg<1,2,18,{io}>"),
       (6, 64, "gn_gelu_fwd_kernel<1>"), (6, 128, "gn_gelu_fwd_kernel<2>"), (5, 256, "gn_gelu_fwd_kernel<4>"),
       (336, 64, "gn_gelu_fwd_kernel<1>"), (100, 64, "gn_gelu_fwd_kernel<1>")]
FWD_Y16 = [(48, 64, "gn_gelu_fwd_reg16<1,3>"), (40, 64, "gn_gelu_fwd_reg16<1,3>"), (96, 64, "gn_gelu_fwd_reg16<1,6>"),
           (24, 256, "gn_gelu_fwd_reg16<4,6>"), (97, 64, "")]
# (L, Cout) -> backward kernel with an fp32 y; `{f}` are the IO16, D16, Y16 template arguments of the register kernel
BWD = [(48, 64, "gn_gelu_bwd_reg<1,4,9,{f}>"), (96, 64, "gn_gelu_bwd_reg<1,8,9,{f}>"), (24, 64, "gn_gelu_bwd_kernel<1>"),
       (40, 64, "gn_gelu_bwd_kernel<1>"), (336, 64, "gn_gelu_bwd_kernel<1>")]
# every tensor bf16, no split pair
BWD_Y16 = [(48, 64, "gn_gelu_bwd_reg<1,4,9,true,true,true>"), (96, 64, "gn_gelu_bwd_reg<1,8,9,true,true,true>"),
           (40, 64, "gn_gelu_bwd_reg16<1,3>"), (97, 64, "")]


@pytest.fixture(scope="module")
def ops():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    from tecmollm import ops
    return ops


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    monkeypatch.delenv("TECM_GN_BWD_SPLIT", raising=False)
    monkeypatch.delenv("TECM_GN_BWD_WPS", raising=False)


def test_forward_paths_are_pinned(ops):
    for L, Cout, want in FWD:
        generic = "reg" not in want
        assert ops.gn_fwd_path(L, 3, Cout) == want.format(io="false"), (L, Cout)
        assert ops.gn_fwd_path(L, 3, Cout, OUT16) == ("" if generic else want.format(io="true")), (L, Cout)
        assert ops.gn_fwd_path(L, 3, Cout, 0, 2) == ("" if generic else want.format(io="false")), (L, Cout)
    for L, Cout, want in FWD_Y16:
        assert ops.gn_fwd_path(L, 3, Cout, Y16 | OUT16) == want, (L, Cout)
        assert ops.gn_fwd_path(L, 3, Cout, Y16 | OUT16, 2) == want, (L, Cout)
        assert ops.gn_fwd_path(L, 3, Cout, Y16 | OUT16 | GIVEN, 2) == "gn_apply_fwd16_kernel", (L, Cout)
    assert ops.gn_fwd_path(336, 3, 72, Y16 | OUT16 | GIVEN) == "gn_apply_fwd16_kernel"       # elementwise: any Cout % 8 == 0
    assert ops.gn_fwd_path(48, 3, 68, Y16 | OUT16 | GIVEN) == ""


def test_forward_refusals_give_no_path(ops):
    for io in (Y16, DACT16, GIVEN, OUT16 | GIVEN, Y16 | GIVEN, ALL16, 16):
        assert ops.gn_fwd_path(48, 3, 64, io) == "", io
    assert ops.gn_fwd_path(48, 3, 64, 0, 0) == ""                 # act_stride < 1
    assert ops.gn_fwd_path(48, 3, 96) == "" and ops.gn_fwd_path(48, 3, 96, Y16 | OUT16) == ""
    assert ops.gn_fwd_path(0, 3, 64) == "" and ops.gn_fwd_path(48, 0, 64) == ""
    assert ops.gn_fwd_path(48, 2 ** 18, 64, Y16 | OUT16) == ""    # 32-bit offsets inside one sample
    assert ops.gn_fwd_path(48, 2 ** 18, 64) == "gn_gelu_fwd_kernel<1>"


def test_backward_paths_are_pinned(ops):
    for L, Cout, want in BWD:
        generic = "reg" not in want
        assert ops.gn_bwd_path(L, 3, Cout) == want.format(f="false,false,false"), (L, Cout)
        assert ops.gn_bwd_path(L, 3, Cout, OUT16) == ("" if generic else want.format(f="true,false,false")), (L, Cout)
        assert ops.gn_bwd_path(L, 3, Cout, OUT16 | DACT16) == ("" if generic else want.format(f="true,true,false")), (L, Cout)
        assert ops.gn_bwd_path(L, 3, Cout, 0, True) == want.format(f="false,false,false"), (L, Cout)   # sums unused: fp32 y
    for L, Cout, want in BWD_Y16:
        assert ops.gn_bwd_path(L, 3, Cout, ALL16, False) == want, (L, Cout)
    # a workspace for the sums: the streaming pair for Cout 64 / 128 whatever L, the register kernels for Cout 256
    for L in (48, 96, 40, 97, 336):
        assert ops.gn_bwd_path(L, 3, 64, ALL16, True) == "gn_bwd_sums16_kernel<1>+gn_bwd_apply16_kernel<1>"
        assert ops.gn_bwd_path(L, 3, 128, ALL16) == "gn_bwd_sums16_kernel<2>+gn_bwd_apply16_kernel<2>"     # ops passes the sums
    assert ops.gn_bwd_path(12, 3, 256, ALL16, True) == "gn_gelu_bwd_reg<4,4,9,true,true,true>"
    assert ops.gn_bwd_path(24, 3, 256, ALL16, True) == "gn_gelu_bwd_reg<4,8,9,true,true,true>"
    assert ops.gn_bwd_path(6, 3, 256, ALL16, True) == "gn_gelu_bwd_reg16<4,3>"
    assert ops.gn_bwd_path(25, 3, 256, ALL16, True) == ""


def test_backward_environment_switches(ops, monkeypatch):
    monkeypatch.setenv("TECM_GN_BWD_SPLIT", "0")
    for L, Cout, want in BWD_Y16:
        assert ops.gn_bwd_path(L, 3, Cout, ALL16, True) == want, (L, Cout)
    # TECM_GN_BWD_WPS=8 skips the 4-wave step: L 48 fits no 8-wave geometry and falls to the oct kernel
    monkeypatch.setenv("TECM_GN_BWD_WPS", "8")
    assert ops.gn_bwd_path(48, 3, 64, ALL16, True) == "gn_gelu_bwd_reg16<1,3>"
    assert ops.gn_bwd_path(96, 3, 64, ALL16, True) == "gn_gelu_bwd_reg<1,8,9,true,true,true>"
    assert ops.gn_bwd_path(48, 3, 64, OUT16) == "gn_gelu_bwd_reg<1,4,9,true,false,false>"      # the switch is the all-bf16 form's
    monkeypatch.delenv("TECM_GN_BWD_SPLIT")
    assert ops.gn_bwd_path(48, 3, 64, ALL16, True) == "gn_bwd_sums16_kernel<1>+gn_bwd_apply16_kernel<1>"
    monkeypatch.setenv("TECM_GN_BWD_SPLIT", "1")
    assert ops.gn_bwd_path(48, 3, 64, ALL16, True) == "gn_bwd_sums16_kernel<1>+gn_bwd_apply16_kernel<1>"


def test_backward_refusals_give_no_path(ops):
    for io in (Y16, DACT16, Y16 | OUT16, Y16 | DACT16, GIVEN, ALL16 | GIVEN, 16):
        assert ops.gn_bwd_path(48, 3, 64, io, True) == "", io
    assert ops.gn_bwd_path(48, 3, 96) == "" and ops.gn_bwd_path(0, 3, 64) == "" and ops.gn_bwd_path(48, 0, 64) == ""


def test_support_queries_agree_with_the_paths(ops):
    h = ops.lib()
    for Cout in (64, 128, 256):
        for L in range(1, 401):
            reg = ops.gn_fwd_path(L, 3, Cout, OUT16) != "" and ops.gn_bwd_path(L, 3, Cout, OUT16) != ""
            assert h.tecm_gn_reg_supported(L, 3, Cout) == int(reg), (L, Cout)
            assert h.tecm_gn_y16_supported(L, 3, Cout) == int(ops.gn_fwd_path(L, 3, Cout, Y16 | OUT16) != ""), (L, Cout)
