"""Host-side limits of long input windows: GPT-2 has 1024 positions (wpe rows), so a model whose trunk would see more
latent-patch tokens is refused when it is built, before its prediction head is allocated."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_cpu as R  # noqa: E402


@pytest.mark.parametrize("L_in,patch_len", [(4100, 1), (8200, 2)], ids=["T1025", "T1025_p2"])
def test_constructor_refuses_more_patches_than_gpt2_positions(L_in, patch_len):
    from src.model.tec_mollm import TEC_MoLLM
    cfg = R.default_config(L_in=L_in, num_nodes=12)
    cfg.update(patch_len=patch_len, include_wte=False, load_pretrained_gpt2=False)
    assert (L_in // 4) // patch_len == 1025
    with pytest.raises(ValueError, match="1024"):
        TEC_MoLLM(cfg)
