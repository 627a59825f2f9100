"""The hard-input suite without a GPU (tests/hard_inputs.py): the families are deterministic and finite, plain fp32
PyTorch stays under BAR / 4 on every case the GPU tests bar against it (so the bars of tests/test_gpu_hard_inputs.py ask
for nothing fp32 cannot give), the activation bars hold for fp32 F.gelu, and the metric and the families catch planted
faults -- each a few lines of fp32 PyTorch -- of the kind a subtly wrong kernel would have."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import hard_inputs as HI  # noqa: E402


def _rng():
    from tecmollm import rng
    return rng


# ------------------------------------------------------------------------------------------------ families
def test_families_are_deterministic_and_finite():
    for fam in HI.NORM_FAMILIES + ("randn",):
        a, b = HI.norm_group(fam, (48, 64), 3), HI.norm_group(fam, (48, 64), 3)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), fam
    x, names = HI.norm_rows(HI.NORM_FAMILIES + ("randn",), 8, 768)
    assert x.shape == (64, 768) and names[0] == "offset" and names[-1] == "randn"
    assert abs(float(x[0].mean()) - HI.LN_OFFSET) < 1 and float(x[40:48].min()) == float(x[40:48].max())   # |mean| >> std; zero variance
    y, names = HI.gn_input(2, 6, 3, 64, 0)
    assert torch.equal(y, HI.gn_input(2, 6, 3, 64, 0)[0]) and bool(torch.isfinite(y).all()) and len(set(names)) == 6
    for fam in HI.SOFTMAX_FAMILIES + ("randn",):
        for T in (1, 13, 130):
            a = HI.softmax_qkv(fam, 2, T, 3)
            assert torch.equal(a, HI.softmax_qkv(fam, 2, T, 3)) and bool(torch.isfinite(a).all()), (fam, T)
            assert bool(torch.isfinite(a.bfloat16().float()).all())
    for bf in (False, True):
        g = HI.act_grid(bf)
        assert g.numel() == 263 and bool(torch.isfinite(g).all()) and float(g.min()) == -40 and float(g.max()) == 40
        assert not bf or torch.equal(g, g.bfloat16().float())
    e, t = HI.huber_errors(4099)
    assert bool(torch.isfinite(e).all()) and int((e.abs() == 1).sum()) >= 2 and int((e == 0).sum()) >= 2


def test_softmax_families_have_the_logits_they_promise():
    T = 24
    for fam, lo, hi in (("peaked3", 2.6, 3.4), ("peaked8", 7.0, 9.0), ("peaked16", 14.0, 18.0)):
        q, k, _ = HI.softmax_qkv(fam, 2, T, 3).view(2, T, 3, 3, HI.H, HI.HD).permute(3, 0, 2, 4, 1, 5)
        assert lo < float(((q @ k.transpose(-1, -2)) / 8).std()) < hi
    logits = {}
    for fam in ("randn", "rising", "falling", "sink", "common_offset"):
        q, k, _ = HI.softmax_qkv(fam, 2, T, 3).view(2, T, 3, 3, HI.H, HI.HD).permute(3, 0, 2, 4, 1, 5)
        logits[fam] = (q @ k.transpose(-1, -2)) / 8                       # (Bn, N, H, query, key)
        assert float(logits[fam].abs().max()) <= HI.LOGIT_CAP + 8
    assert float(logits["randn"].abs().max()) < 8
    step = logits["rising"][..., 1:] - logits["rising"][..., :-1]         # slope 1 per key, to every query alike
    assert abs(float(step.mean()) - 1) < 0.05 and float((logits["rising"][..., 23] - logits["rising"][..., 0]).min()) > 23 - 8
    step = logits["falling"][..., 1:] - logits["falling"][..., :-1]
    assert abs(float(step.mean()) + 1) < 0.05 and float((logits["falling"][..., 0] - logits["falling"][..., 23]).min()) > 23 - 8
    assert float((logits["sink"][..., 0] - logits["sink"][..., 1:].max(-1).values).min()) > HI.SINK - 8
    assert abs(float(logits["common_offset"].mean()) - HI.COMMON_OFFSET) < 0.1 and float(logits["common_offset"].min()) > HI.COMMON_OFFSET - 8
    # cliff: to every query from 32 on, the first 16 keys lie so far below the rest that exp(m_old - m_new) is 0 in fp32;
    # the earlier queries, and every short sequence, see plain logits
    T = 65
    q, k, _ = HI.softmax_qkv("cliff", 2, T, 3).view(2, T, 3, 3, HI.H, HI.HD).permute(3, 0, 2, 4, 1, 5)
    w = (q @ k.transpose(-1, -2)) / 8
    late = w[..., HI.CLIFF_QUERY:, :]
    gap = late[..., HI.CLIFF_KEYS:HI.CLIFF_QUERY].max(-1).values - late[..., :HI.CLIFF_KEYS].max(-1).values
    assert float(gap.min()) > 104 and float(torch.exp(-gap).max()) == 0.0
    assert float(w[..., :HI.CLIFF_QUERY, :].abs().max()) < 8 and float(late[..., HI.CLIFF_KEYS:].abs().max()) < 8


# ------------------------------------------------------------------------------------------------ fp32 stays under BAR / 4
def _assert_cpu(rows):
    bad = [f"{lab}: need_cpu {nc:.3g}" for lab, nc in rows if not nc <= HI.BAR / 4]
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("shape", [s[0] for s in HI.LN_SHAPES])
def test_fp32_layernorm_stays_under_a_quarter_of_the_bar(shape):
    rows = []
    for inst in (HI.LN_BWD if shape == "mixed768" else ("plain",)):
        cpu, ref = HI.ln_refs(shape, inst, _rng())
        rows += [(lab, HI.need(c, r, dims)) for lab, _, c, r, dims in HI.ln_entries(cpu, cpu, ref, f"{shape}/{inst}/")]
    _assert_cpu(rows)


@pytest.mark.parametrize("name", list(HI.GN_SHAPES))
def test_fp32_groupnorm_gelu_stays_under_a_quarter_of_the_bar(name):
    cpu, ref, (*_, names) = HI.gn_refs(name)
    assert "offset" in names and "constant" in names                      # every kernel family sees |mean| >> std and zero variance
    Cout = HI.GN_SHAPES[name][0][3]
    rows = [(lab, HI.need(c, r, dims)) for lab, _, c, r, dims in HI.gn_entries(cpu, cpu, ref, Cout, name + "/")]
    _assert_cpu(rows)


@pytest.mark.parametrize("T", HI.ATT_SHORT + HI.ATT_LONG)
def test_fp32_attention_stays_under_a_quarter_of_the_bar(T):
    rows = []
    for fam in HI.SOFTMAX_FAMILIES:
        for inst in HI.ATT_INST:
            cpu, ref = HI.att_refs(fam, T, inst, _rng(), "cpu")
            for nm, c, r in zip(("ctx", "dqkv"), cpu, ref):
                if c is not None:
                    rows.append((f"{fam}/T{T}/{inst}/{nm}", HI.need(HI.att_heads(c), HI.att_heads(r), (-1,))))
    _assert_cpu(rows)


@pytest.mark.parametrize("variation", HI.SPATIAL_VARIATIONS)
@pytest.mark.parametrize("graph", HI.SPATIAL_GRAPHS)
def test_fp32_oracle_stays_under_a_quarter_of_the_bar_on_the_spatial_stage(graph, variation):
    from oracle import ref_cpu as R
    p, x, tf, ei, gout = HI.spatial_inputs(R, graph, variation)
    cpu, ref = HI.spatial_oracle(R, p, x, tf, ei, gout, torch.float32), HI.spatial_oracle(R, p, x, tf, ei, gout, torch.float64)
    rows = [("out", HI.need(cpu[0], ref[0], (-1,))), ("dx", HI.need(cpu[2], ref[2], (-1,)))]
    rows += [(n, HI.need(c, r, None)) for n, c, r in zip(HI.spatial_names(R), cpu[1], ref[1])]
    _assert_cpu(rows)


def test_closed_form_softmax_backward_needs_its_dalpha_shifted():
    """The planted fault the GATv2 backward kernels had: de = alpha (dalpha - sum alpha dalpha) with dalpha as it comes, in
    plain fp32, misses BAR on the d lin_r gradients once every source carries a common offset; shifted by the self loop's
    dalpha it passes the bars the GPU tests hold the kernels to (BAR, and K times what autograd's chain needs)."""
    from oracle import ref_cpu as R
    p, x, tf, ei, gout = HI.spatial_inputs(R, "grid", "xoff")
    names = HI.spatial_names(R)
    cpu = HI.spatial_oracle(R, p, x, tf, ei, gout, torch.float32)
    ref = HI.spatial_oracle(R, p, x, tf, ei, gout, torch.float64)
    ib, iw = names.index(R.P_GAT + "lin_r.bias"), names.index(R.P_GAT + "lin_r.weight")
    b64, w64 = HI.gat_closed_form(R, p, x, tf, ei, gout, torch.float64, "plain")
    assert HI.need(b64, ref[1][ib], None) < 1e-9 and HI.need(w64, ref[1][iw], None) < 1e-9     # the closed form is the gradient
    plain = HI.gat_closed_form(R, p, x, tf, ei, gout, torch.float32, "plain")
    shift = HI.gat_closed_form(R, p, x, tf, ei, gout, torch.float32, "shift")
    for got_p, got_s, i in ((plain[0], shift[0], ib), (plain[1], shift[1], iw)):
        auto = HI.need(cpu[1][i], ref[1][i], None)
        n_p, n_s = HI.need(got_p, ref[1][i], None), HI.need(got_s, ref[1][i], None)
        print(names[i], "autograd", auto, "closed form", n_p, "shifted", n_s)
        assert n_p > HI.BAR and not HI.passes(n_p, auto)
        assert n_s <= HI.BAR / 4 and HI.passes(n_s, auto)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("tanh", [True, False], ids=["tanh", "erf"])
def test_fp32_gelu_meets_the_activation_bars_on_the_grid(tanh, bf16):
    """The three bars of the activation sweep are ones plain fp32 F.gelu and its derivative meet on the same grid."""
    g = HI.act_grid(bf16)
    ref, dref = HI.gelu_ref(g.double(), tanh), HI.dgelu_ref(g.double(), tanh)
    x = g.clone().requires_grad_(True)
    act = F.gelu(x, approximate="tanh" if tanh else "none")
    (d,) = torch.autograd.grad(act.sum(), x)
    assert bool(((act.detach().double() - ref).abs() <= HI.ACT_ABS + HI.ACT_REL * ref.abs()).all())
    assert bool(((d.double() - dref).abs() <= HI.DACT_ABS).all())
    a16 = act.detach().bfloat16().double()
    assert bool(((a16 - ref).abs() <= 2.0 ** -7 * ref.abs() + 1e-6).all())
    big, neg = g >= 10, g <= -10
    assert torch.equal(act.detach()[big], g[big]) and float(act.detach()[neg].abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------------ planted faults
def _ln_one_pass(x, gamma, beta):
    mean = x.mean(-1, keepdim=True)
    var = (x * x).mean(-1, keepdim=True) - mean * mean                   # cancels when |mean| >> std
    return (x - mean) / torch.sqrt(var + HI.EPS) * gamma + beta


def test_a_one_pass_variance_fails_offset_and_passes_randn():
    gamma, beta = HI.affine(768, 2)
    for fam, fails in (("offset", True), ("randn", False)):
        x, _ = HI.norm_rows((fam,), 8, 768)
        ref = F.layer_norm(x.double(), (768,), gamma.double(), beta.double(), HI.EPS)
        n = HI.need(_ln_one_pass(x, gamma, beta), ref, (-1,))
        n_ok = HI.need(F.layer_norm(x, (768,), gamma, beta, HI.EPS), ref, (-1,))
        assert (n > HI.BAR) == fails, (fam, n)
        assert HI.passes(n, n_ok) == (not fails), (fam, n, n_ok)


def test_a_softmax_without_max_subtraction_is_not_finite_on_peaked():
    T = 130                                                               # 1.2 M logits of std 16: the largest is past 88.7
    qkv = HI.softmax_qkv("peaked16", 2, T, 3)
    q, k, v = qkv.view(2, T, 3, 3, HI.H, HI.HD).permute(3, 0, 2, 4, 1, 5)
    w = (q @ k.transpose(-1, -2)) / 8
    e = torch.exp(w) * torch.tril(torch.ones(T, T))
    out = (e / e.sum(-1, keepdim=True)) @ v
    assert not bool(torch.isfinite(out).all())
    assert HI.need(out, HI.attention_ref(qkv.double(), 2, T, 3).view(2, T, 3, HI.H, HI.HD).permute(0, 2, 3, 1, 4), (-1,)) == float("inf")
    qkv = HI.softmax_qkv("randn", 2, T, 3)                                # ... and is fine on the inputs the suite had
    q, k, v = qkv.view(2, T, 3, 3, HI.H, HI.HD).permute(3, 0, 2, 4, 1, 5)
    e = torch.exp((q @ k.transpose(-1, -2)) / 8) * torch.tril(torch.ones(T, T))
    assert bool(torch.isfinite((e / e.sum(-1, keepdim=True)) @ v).all())


def _online_softmax(qkv, T, rescale_acc, step=16):
    """Causal attention by an online softmax over `step`-key tiles in fp32; rescale_acc = False drops the alpha factor of
    the accumulator (the running sum keeps it)."""
    q, k, v = qkv.view(2, T, 3, 3, HI.H, HI.HD).permute(3, 0, 2, 4, 1, 5)
    w = ((q @ k.transpose(-1, -2)) / 8).masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), float("-inf"))
    m = torch.full(w.shape[:-1] + (1,), float("-inf"))
    s = torch.zeros_like(m)
    acc = torch.zeros(w.shape[:-1] + (HI.HD,))
    for j0 in range(0, T, step):
        blk = w[..., j0:j0 + step]
        mn = torch.maximum(m, blk.max(-1, keepdim=True).values)
        mn = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)       # rows that have seen no key yet
        alpha = torch.exp(m - mn)
        p = torch.exp(blk - mn)
        s = s * alpha + p.sum(-1, keepdim=True)
        acc = (acc * alpha if rescale_acc else acc) + p @ v[..., j0:j0 + step, :]
        m = mn
    return (acc / s).permute(0, 3, 1, 2, 4).reshape(2, T, 3, HI.D)


def test_a_dropped_alpha_fails_rising_and_cliff_and_passes_falling():
    T = 65
    for fam, fails in (("rising", True), ("cliff", True), ("falling", False)):
        qkv = HI.softmax_qkv(fam, 2, T, 3)
        ref = HI.att_heads(HI.attention_ref(qkv.double(), 2, T, 3))
        good = HI.need(HI.att_heads(_online_softmax(qkv, T, True)), ref, (-1,))
        bad = HI.need(HI.att_heads(_online_softmax(qkv, T, False)), ref, (-1,))
        cpu = HI.need(HI.att_heads(HI.attention_ref(qkv, 2, T, 3)), ref, (-1,))
        assert good <= HI.BAR / 4 and HI.passes(good, max(cpu, good / HI.K))
        assert (bad > HI.BAR) == fails, (fam, bad)
    # on randn inputs the fault is there too, but a max-norm over the whole tensor shrinks it; the row metric does not
    qkv = HI.softmax_qkv("rising", 2, T, 3)
    ref = HI.attention_ref(qkv.double(), 2, T, 3)
    bad = _online_softmax(qkv, T, False)
    assert HI.need(HI.att_heads(bad), HI.att_heads(ref), (-1,)) > 10 * float((bad.double() - ref).abs().max() / ref.abs().max())


def test_statistics_shared_between_neighbouring_rows_fail_mixed():
    x, names = HI.norm_rows(HI.NORM_FAMILIES + ("randn",), 8, 768)
    gamma, beta = HI.affine(768, 2)
    ref = F.layer_norm(x.double(), (768,), gamma.double(), beta.double(), HI.EPS)
    _, mean, rstd = torch.native_layer_norm(x, (768,), gamma, beta, HI.EPS)          # the statistics F.layer_norm forms
    own = (x - mean) * rstd * gamma + beta
    assert HI.need(own, ref, (-1,)) <= HI.BAR / 4
    # one slot for every 8 rows, written by the last of them
    slot = torch.arange(64) // 8 * 8 + 7
    shared = (x - mean[slot]) * rstd[slot] * gamma + beta
    assert HI.need(shared, ref, (-1,)) > HI.BAR
    # a slot shared across a family boundary (row 7 | row 8) fails by orders of magnitude, not by a rounding
    slot = torch.arange(64)
    slot[8] = 7
    leak = (x - mean[slot]) * rstd[slot] * gamma + beta
    per_row = HI.need_map(leak, ref, (-1,)).max(-1).values
    assert float(per_row[8]) > 100 * HI.BAR and float(per_row[torch.arange(64) != 8].max()) <= HI.BAR / 4


def test_an_unclamped_tanh_gelu_is_nan_at_40():
    x = HI.act_grid()
    u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
    E = torch.exp(2 * u)
    bad = x * (E / (1 + E))                                              # inf / inf
    assert bool(torch.isnan(bad[x == 40]).all())
    clamped = torch.clamp(E, max=2.0 ** 100)
    good = x * (clamped / (1 + clamped))
    ref = HI.gelu_ref(x.double(), True)
    assert bool(torch.isfinite(good).all()) and bool(((good.double() - ref).abs() <= 2 * HI.ACT_ABS + 4 * HI.ACT_REL * ref.abs()).all())


def test_metric_judges_small_entries_on_the_scale_of_their_row():
    ref = torch.tensor([[1000.0, 1.0, 2.0], [0.001, 0.002, 0.003]]).double()
    got = ref.clone()
    got[1, 0] *= 1.5                                                      # a 50 % error in a small row of a tensor with a large entry
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-6        # invisible to a max-norm ratio
    assert HI.need(got, ref, (-1,)) > 1e-4
    assert HI.need(ref, ref, (-1,)) == 0.0
    got[0, 0] = float("nan")
    assert HI.need(got, ref, (-1,)) == float("inf")
    assert HI.need(torch.zeros(3), torch.zeros(3), None) == 0.0
