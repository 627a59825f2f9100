"""Host side of activation recomputation (tecmollm/memory.py): the bytes the autograd stages keep for their backward, the
step estimate for a table of configurations, and the policy that picks the recompute level of a forward."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_cpu as R  # noqa: E402

LIB = os.path.join(ROOT, "tec-mollm_amd", "tecmollm", "libtecmollm_hip.so")
GB = 1e9
N = 2911


@pytest.fixture(scope="module")
def mem():
    if not os.path.exists(LIB):                      # the storage policy asks the library which kernels serve a shape
        import __graft_entry__ as g
        g.build()
    from tecmollm import memory
    return memory


def _cfg(L_in):
    return R.default_config(L_in=L_in, L_out=12, num_nodes=N, c_in=10, d_emb=12)


def test_bytes_kept_per_token_and_per_step(mem):
    """Level 0, per token and GPT-2 block: h, u, st1, qkv, h2, st2, a (fp32: 30 864 B); bf16 mode in training adds the bf16
    LoRA input u16d and halves u, qkv and a (20 048 B).  Per (input step, node) of one sample, both conv blocks at the timed
    window (compact activations behind the stride-2 1x1 convs): inp, y and act, 2 528 B in fp32.  Per sample and L_in step at
    N = 2911 with patch_len 4 (T = L_in / 16): about 24 MB in fp32, 16 MB in bf16 mode."""
    assert mem.layer_bytes_per_token(0, True) == 30864
    assert mem.layer_bytes_per_token(0, False) == 30864
    assert mem.layer_bytes_per_token(1, True) == 20048
    assert mem.layer_bytes_per_token(1, False) == 20048 - 1536
    c48 = _cfg(48)
    assert mem.conv_bytes_per_step(c48, 0) == 2528
    b16 = mem.conv_bytes_per_step(c48, 1)
    assert 1400 <= b16 <= 1900, b16
    for prec, want in ((0, 24e6), (1, 16e6)):
        per_step = (3 * mem.layer_bytes_per_token(prec, True) / 16 + mem.conv_bytes_per_step(c48, prec)) * N
        assert abs(per_step / want - 1) < 0.06, (prec, per_step)


# (L_in, B, prec, level, training, grad) -> (kept GB, peak GB) of the estimate, pinned
TABLE = {
    (48, 8, 0, 0, True, True): (9.97, 13.10),
    (48, 8, 0, 2, True, True): (1.57, 6.00),
    (48, 8, 1, 0, True, True): (6.37, 8.20),
    (720, 2, 0, 0, True, True): (40.61, 53.52),
    (720, 2, 0, 1, True, True): (18.78, 36.55),
    (720, 2, 0, 2, True, True): (5.90, 23.67),
    (720, 2, 1, 0, True, True): (32.30, 39.77),
    (720, 2, 1, 2, True, True): (6.10, 17.20),
    (720, 2, 0, 0, False, True): (40.61, 51.91),
    (720, 2, 0, 0, False, False): (2.01, 10.06),
}


def test_estimate_table(mem):
    for (L_in, B, prec, lv, tr, gr), (kept, peak) in TABLE.items():
        e = mem.estimate(_cfg(L_in), B, prec, lv, tr, gr)
        assert abs(e.kept / GB - kept) <= 0.01 * kept + 0.02, ((L_in, B, prec, lv, tr, gr), e)
        assert abs(e.peak / GB - peak) <= 0.01 * peak + 0.02, ((L_in, B, prec, lv, tr, gr), e)
    for L_in, B in ((48, 8), (720, 2), (1440, 8)):
        for prec in (0, 1):
            for tr in (True, False):
                est = [mem.estimate(_cfg(L_in), B, prec, lv, tr, True) for lv in (0, 1, 2)]
                assert est[0].kept > est[1].kept > est[2].kept
                assert est[0].peak > est[1].peak > est[2].peak
                lean = [mem.estimate(_cfg(L_in), B, prec, lv, tr, False) for lv in (0, 1, 2)]
                assert lean[0] == lean[1] == lean[2]                  # no backward: the level does not matter
                assert lean[0].peak < est[2].peak
            assert mem.estimate(_cfg(L_in), B, 1, 0, True, True).kept < mem.estimate(_cfg(L_in), B, 0, 0, True, True).kept
    # the configurations that do not fit a 288 GB device at level 0
    assert mem.estimate(_cfg(1440), 8, 0, 0, True, True).peak > 288 * GB
    assert mem.estimate(_cfg(1440), 8, 0, 2, True, True).peak < 200 * GB
    assert mem.estimate(_cfg(1440), 16, 0, 0, False, False).peak < 200 * GB


def test_policy_keeps_level_0_where_it_fits_and_recomputes_below(mem):
    total = 288 * GB
    budget = total - mem.margin(total)
    for prec in (0, 1):
        est = lambda lv, prec=prec: mem.estimate(_cfg(48), 8, prec, lv, True, True)   # noqa: E731
        assert mem.pick(est, budget) == 0                       # the benchmark configuration
    est = lambda lv: mem.estimate(_cfg(720), 2, 0, lv, True, True)                     # noqa: E731
    p0, p1, p2 = (est(lv).peak for lv in (0, 1, 2))
    assert mem.pick(est, p0) == 0
    assert mem.pick(est, p0 - 1) == 1
    assert mem.pick(est, p1 - 1) == 2
    assert mem.pick(est, p2 - 1) == 2                           # nothing fits: the smallest there is
    assert mem.pick(est, p2) == 2


def test_the_diagnostic_variable_forces_a_level_or_a_budget_and_decisions_are_cached(mem, monkeypatch):
    calls = []

    def est(lv):
        calls.append(lv)
        return mem.Estimate(kept=(3 - lv) * 10, transient=5)
    mem.clear_choices()
    for v, want in (("0", 0), ("1", 1), ("2", 2)):
        monkeypatch.setenv(mem.ENV, v)
        assert mem.choose(("k",), est, None) == want
        assert mem.choose(("k",), est, None, levels=(0, 1)) == min(want, 1)
    assert calls == []                                          # a forced level estimates nothing
    monkeypatch.setenv(mem.ENV, "budget:0.000000026")          # 26 bytes: level 1 (25) fits, level 0 (35) does not
    assert mem.choose(("k",), est, None) == 1
    n = len(calls)
    assert mem.choose(("k",), est, None) == 1 and len(calls) == n        # cached per key
    monkeypatch.setenv(mem.ENV, "budget:0.000000015")
    assert mem.choose(("k",), est, None) == 2
    monkeypatch.setenv(mem.ENV, "sometimes")
    with pytest.raises(ValueError):
        mem.choose(("k",), est, None)
    mem.clear_choices()


def test_plan_carries_the_level_and_checkpointing_stays_harmless():
    from src.model import modules as M_
    from tecmollm import functions as F_
    plan = F_.DropPlan(True, 0.1, 7)
    assert plan.recompute == 0 and plan.keep
    bb = M_.LLMBackbone(num_layers_to_keep=1, include_wte=False, load_pretrained=False)
    assert bb.model.gradient_checkpointing_enable() is None
    assert "recomput" in M_._PeftGPT2.gradient_checkpointing_enable.__doc__
