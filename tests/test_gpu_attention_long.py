"""The long-window attention kernels (csrc/attention_long.hip, 33 <= T <= 1024 tokens per sequence) against float64:
every forward and backward input-type instance, dropout off and on, into NaN-filled outputs, bf16 outputs equal to the
round-to-nearest-even of the fp32 ones; bit-identical repeated launches of a grid larger than one wave of blocks; and the
T = 1025 refusal."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests.test_gpu_ops import ATT_BWD, _assert_att, _att_case  # noqa: E402

pytestmark = pytest.mark.gpu

H, D = 12, 768
# 33: first long length; 45: L_in = 180 / 720; 63..65, 127..129: either side of the 64-key tile steps; 1024: GPT-2's last
LENGTHS = [33, 34, 40, 45, 63, 64, 65, 96, 127, 128, 129, 200, 256, 333, 512, 1024]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _shape(T):
    """(Bn, N): the float64 reference and the mirrored mask grow with Bn*N*12*T^2 -- 25 M scores at T = 1024, Bn*N = 2"""
    return (2, 3) if T <= 200 else (1, 2)


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop"])
@pytest.mark.parametrize("inst", list(ATT_BWD))
@pytest.mark.parametrize("T", LENGTHS)
def test_long_attention_matches_float64(dev, T, inst, p):
    from tecmollm import ops
    q16, d16 = ATT_BWD[inst]
    Bn, N = _shape(T)
    q_in, d_in, drop, ref, gref = _att_case(dev, Bn, T, N, q16, d16, p)
    nan = float("nan")
    if not d16:                                     # the forward reads qkv only: once per forward instance
        ctx = torch.full(ref.shape, nan, device=dev)
        ops.attention_fwd(q_in, ctx, Bn, T, N, H, D, drop)
        _assert_att(ctx, ref, "ctx")
        ctx16 = torch.full(ref.shape, nan, device=dev, dtype=torch.bfloat16)
        ops.attention_fwd(q_in, ctx16, Bn, T, N, H, D, drop)
        assert torch.equal(ctx16, ctx.bfloat16())
    dq = torch.full(q_in.shape, nan, device=dev)
    ops.attention_bwd(q_in, d_in, dq, Bn, T, N, H, D, drop)
    _assert_att(dq, gref, "dqkv")
    dq16 = torch.full(q_in.shape, nan, device=dev, dtype=torch.bfloat16)
    ops.attention_bwd(q_in, d_in, dq16, Bn, T, N, H, D, drop)
    assert torch.equal(dq16, dq.bfloat16())


# 2 * 400 * 12 = 9 600 (sequence, head) problems: the backward's 9 600 workgroups and the forward's 9 600 * ceil(T/16)
# waves are several waves of blocks on 256 CUs.  Three launches into NaN-filled buffers: complete, bit-identical, right.
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop"])
@pytest.mark.parametrize("inst", list(ATT_BWD))
@pytest.mark.parametrize("T", [45, 64, 128])
def test_long_attention_reproducible(dev, T, inst, p):
    from tecmollm import ops
    q16, d16 = ATT_BWD[inst]
    Bn, N = 2, 400
    q_in, d_in, drop, ref, gref = _att_case(dev, Bn, T, N, q16, d16, p)
    if not d16:
        outs = [torch.full(ref.shape, float("nan"), device=dev) for _ in range(3)]
        for o in outs:
            ops.attention_fwd(q_in, o, Bn, T, N, H, D, drop)
        assert not bool(torch.isnan(outs[0]).any())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        _assert_att(outs[0], ref, "ctx")
    outs = [torch.full(q_in.shape, float("nan"), device=dev) for _ in range(3)]
    for o in outs:
        ops.attention_bwd(q_in, d_in, o, Bn, T, N, H, D, drop)
    assert not bool(torch.isnan(outs[0]).any())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    _assert_att(outs[0], gref, "dqkv")


def test_t_above_gpt2_positions_is_refused(dev):
    from tecmollm import TecmError, ops
    T, Bn, N = 1025, 1, 1
    qkv = torch.zeros(Bn, T, N, 3 * D, device=dev)
    with pytest.raises(TecmError, match="1024"):
        ops.attention_fwd(qkv, torch.zeros(Bn, T, N, D, device=dev), Bn, T, N, H, D)
    with pytest.raises(TecmError, match="1024"):
        ops.attention_bwd(qkv, torch.zeros(Bn, T, N, D, device=dev), torch.zeros_like(qkv), Bn, T, N, H, D)
