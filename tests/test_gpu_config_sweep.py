"""One full training step (forward, loss, all gradients) against the CPU oracle over model configurations the reference's
ctor accepts and the timed configurations do not touch: sequence lengths 8..96, channel lists, strides, patch lengths,
feature widths, layer counts -- in fp32 and bf16 mode, eval and train (tools/config_sweep.py as a test: a regression fails
here instead of landing in a profile file).  The problems are tiny (12 nodes = 24 sequences) so that the CPU oracle
finishes in seconds; fp32 takes the standard bars, bf16 the stated 24-sequence bars of tests/parity.py."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_cpu as R  # noqa: E402
from tests.parity import assert_parity, compare_forward_backward  # noqa: E402

pytestmark = pytest.mark.gpu

# (tools/config_sweep.py walks the full matrix -- eight sequence lengths, four (precision, mode) pairs: profiles/r05_config_sweep.txt;
#  the test keeps the lengths that take different kernel routes and the two train-mode pairs -- eval is the same kernels
#  with the mask multiply off -- to stay well inside a minute of GPU time)
CASES = [(f"L{L_in}_{L_out}", dict(L_in=L_in, L_out=L_out), {}) for L_in, L_out in
         ((16, 4), (40, 12), (80, 12), (96, 24), (8, 2))] + [
    ("ch128_256", dict(), {"temporal_channel_list": [128, 256]}),
    ("ch64_64", dict(), {"temporal_channel_list": [64, 64]}),
    # shapes whose fp32 sequence tiles do NOT fit the LDS (tecm_conv_*_supported says no): the window-GEMM fallback serves them
    ("ch64_256_L96", dict(L_in=96, L_out=24), {"temporal_channel_list": [64, 256]}),
    ("ch128_128_L96", dict(L_in=96, L_out=24), {"temporal_channel_list": [128, 128]}),
    ("strides1_2", dict(), {"temporal_strides": [1, 2], "patch_len": 4}),
    ("patch2", dict(), {"patch_len": 2}),
    ("F10", dict(c_in=10, d_emb=12), {}),
    ("layers1", dict(llm_layers=1), {}),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


@pytest.mark.parametrize("prec,train", [("fp32", True), ("bf16", True)], ids=["fp32-train", "bf16-train"])
@pytest.mark.parametrize("name,kw,over", CASES, ids=[c[0] for c in CASES])
def test_full_step_over_model_configurations(dev, name, kw, over, prec, train):
    cfg = R.default_config(num_nodes=12, **kw)
    cfg.update(over)
    res = compare_forward_backward(cfg, B=2, grid=(3, 4), threshold_km=170.0, gat_graphs="per_timestep", seed=5, train=train,
                                   precision=prec)
    if prec == "fp32":
        assert_parity(res)
    else:
        assert_parity(res, small24=True)


# Widths the conv sequence kernels' predicates admit in part -- and the model does not: Multi_Scale_Conv_Block takes out_channels
# 64, 128 and 256 only (the GroupNorm kernels work on 64-channel chunks) and says so when it is built.  No full step exists to
# compare; what is pinned is the loud refusal, and what the predicates would route where.
REFUSED_CHANNEL_LISTS = [("ch32_96", {"temporal_channel_list": [32, 96]}), ("ch64_192", {"temporal_channel_list": [64, 192]})]


@pytest.mark.parametrize("name,over", REFUSED_CHANNEL_LISTS, ids=[c[0] for c in REFUSED_CHANNEL_LISTS])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_channel_widths_the_groupnorm_stage_is_not_built_for_fail_loudly(dev, name, over, prec):
    """temporal_channel_list [32, 96] and [64, 192]: the model's constructor raises, naming out_channels, before any kernel runs --
    the stage neither falls back nor mis-computes.  The conv kernels' instantiations for 32, 96 and 192 channels are therefore
    reached through the C ABI only (tests/test_gpu_conv_seq_domain.py)."""
    cfg = R.default_config(num_nodes=12)
    cfg.update(over)
    with pytest.raises(ValueError, match="out_channels must be 64, 128 or 256"):
        compare_forward_backward(cfg, B=2, grid=(3, 4), threshold_km=170.0, gat_graphs="per_timestep", seed=5, precision=prec)


@pytest.mark.parametrize("chans,fwd,dx,dw", [([32, 96], (True, True), (False, False), (False, False)),
                                             ([64, 192], (True, False), (True, True), (True, False))],
                         ids=["ch32_96", "ch64_192"])
def test_channel_lists_meet_the_kernels_their_names_promise(dev, chans, fwd, dx, dw):
    """What WOULD serve the two conv blocks of ch32_96 and ch64_192 at the sweep's shapes (L_in = 48, strides 2, 2; block 0 reads
    the 22 spatial channels at a pitch of 24), in fp32 and in bf16 alike: [32, 96] runs the forward's 3- and 9-unit
    assignments and takes the window-view GEMMs for both gradients (the d-input kernel wants multiples of 64, the
    weight-gradient kernel its four built pairs); [64, 192] runs the d-input kernel at 192 channels and takes the GEMMs for
    the forward (more than 128 channels) and the weight gradient of its second block."""
    from tecmollm import ops
    cfg = R.default_config(num_nodes=12)
    L = cfg["temporal_seq_len"]
    blocks = [(L, chans[0], 24), (L // cfg["temporal_strides"][0], chans[1], chans[0])]
    for f32 in (True, False):
        assert tuple(ops.conv_fwd_seq_ok(*b, f32=f32) for b in blocks) == fwd
        assert tuple(ops.conv_dx_seq_ok(*b, f32=f32) for b in blocks) == dx
    assert tuple(ops.conv_dw_seq_ok(*b) for b in blocks) == dw


def test_unsupported_feature_width_fails_loudly(dev):
    """C = C_in + d_emb != 22 is the one configuration the kernels are not built for: it must raise, not mis-compute."""
    from tecmollm import TecmError
    cfg = R.default_config(num_nodes=12, c_in=4, d_emb=8)
    with pytest.raises((TecmError, ValueError, RuntimeError)):
        compare_forward_backward(cfg, B=2, grid=(3, 4), threshold_km=170.0, gat_graphs="per_timestep", seed=5, precision="fp32")
