"""The whole training step at input windows whose GPT-2 trunk sees more than 32 latent-patch tokens (the long-window
attention of csrc/attention_long.hip): against the CPU oracle with mirrored dropout masks on small graphs, and on the full
graph (N = 2911) as one batch against the mean of its single samples."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_cpu as R  # noqa: E402
from tests.parity import (assert_batch_equals_mean_of_samples, assert_parity, batch_vs_single_sample_grads,  # noqa: E402
                          compare_forward_backward)

pytestmark = pytest.mark.gpu

# L_in = 180 (15 days): L_in // 4 = 45 is odd, so the reference's fallback gives patch_len = 1 and T = 45 (train.py:251-260),
# and conv block 1 runs at Lc = 180.  L_in = 528 (22 days) with patch_len = 4: T = 33, the first long length.
CASES = [("L180_T45", dict(L_in=180, L_out=12), {}), ("L528_T33", dict(L_in=528, L_out=12), {"patch_len": 4})]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name,kw,over", CASES, ids=[c[0] for c in CASES])
def test_long_window_step_matches_oracle(dev, name, kw, over, prec):
    cfg = R.default_config(num_nodes=12, **kw)
    cfg.update(over)
    assert (cfg["temporal_seq_len"] // 4) // cfg["patch_len"] > 32
    res = compare_forward_backward(cfg, B=2, grid=(3, 4), threshold_km=170.0, gat_graphs="per_timestep", seed=5, train=True,
                                   precision=prec)
    if prec == "fp32":
        assert_parity(res)
    else:
        assert_parity(res, small24=True)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_long_window_full_graph_batch_equals_mean_of_samples(dev, prec):
    """L_in = 720 (60 days, T = 45), N = 2911, B = 2, eval mode: the new kernels at real grid sizes, without a CPU run."""
    cfg = R.default_config(L_in=720, L_out=12, num_nodes=2911, c_in=10, d_emb=12)
    assert cfg["patch_len"] == 4 and (720 // 4) // 4 == 45
    assert_batch_equals_mean_of_samples(batch_vs_single_sample_grads(cfg, 2, (41, 71), seed=47, precision=prec))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
