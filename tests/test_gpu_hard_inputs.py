"""The norm, softmax, activation, loss and optimizer kernels on hard-valued inputs (tests/hard_inputs.py): rows with
|mean| >> std, outlier channels, zero variance, near one-hot and steadily rising softmax rows, activation arguments out to
+-40, errors on the Huber kink, gradients that underflow or dwarf the rest.  Every result is compared with float64 on exactly
the values the kernel reads, under the row-relative metric `need`, against BAR = 1e-3 and against K times what plain fp32
PyTorch needs on the same input (FLOOR where that is exact); tests/test_host_hard_inputs.py shows that fp32 stays under
BAR / 4 on every case and that planted faults fail, profiles/hard_inputs.txt has the measured table.  Outputs go into
NaN-filled buffers."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_cpu as R  # noqa: E402
from oracle import shell_cpu as S  # noqa: E402
from tests import gemm_epilogue_cases as GC  # noqa: E402
from tests import hard_inputs as HI  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda")


def _check(entries):
    rows = HI.measure(entries)
    for lab, nc, ng in rows:
        print(f"{lab:58s} need_cpu {nc:9.3g} need_gpu {ng:9.3g} bar {HI.bar_in_force(nc):9.3g}")
    bad = HI.failures(rows)
    assert rows and not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("shape", [s[0] for s in HI.LN_SHAPES])
def test_layernorm_on_hard_rows(dev, shape):
    """64 rows of eight families in one launch at D = 768 (every backward instance: plain, the add= stream fp32 and bf16, a
    bf16 dy, the sequence-major dy), |mean| >> std at D = 256, outlier channels at D = 1024: y, (mean, rstd), dx, dgamma, dbeta."""
    from tecmollm import ops, rng
    entries, extras, names = HI.ln_run(ops, rng, dev, shape, HI.LN_BWD if shape == "mixed768" else ("plain",))
    if shape == "mixed768":
        assert extras["constant_dx_finite"]
        assert extras["constant_y_vs_beta"] <= HI.FLOOR, extras           # zero variance: y is beta
    _check(entries)


# ------------------------------------------------------------------------------------------------ GroupNorm(1) + GELU
@pytest.mark.parametrize("name", list(HI.GN_SHAPES))
def test_groupnorm_gelu_on_hard_sequences(dev, name):
    """One shape per kernel family of csrc/groupnorm.hip (generic, 4- and 8-wave register, Cout = 256, the all-bf16 kernels, Cout =
    256 among them), every sequence of the launch of another family, an `offset` and a `constant` one in every launch, the
    three branches of an offset sequence at different offsets: act, (mean,
    rstd), dy, dgamma, dbeta, colsum(dy).  The all-bf16 kernels' act / dy: one bf16 ulp plus the bar on the group's scale."""
    from tecmollm import ops
    entries, extras, names = HI.gn_run(ops, dev, name)
    print(names, extras)
    assert "offset" in names and "constant" in names
    assert all(v <= 1.0 for v in extras.values()), extras
    _check(entries)


def test_conv_forward_statistics_with_mean_far_above_std(dev):
    """TecmConvFwd.stats merges per-unit (mean, M2) because sums of squares cancel when |mean| >> std: here they would.  The
    elementwise forward that takes these statistics as given (gn_apply_fwd16) then norms such a y: its bf16 act within one
    bf16 ulp plus the bar on the group's scale."""
    from tecmollm import ops, rng
    entries, extras = HI.conv_stats_run(ops, rng, dev)
    print(extras)
    assert extras["conv_stats/min |mean| / std"] > 10
    assert extras["conv_stats/act_bf16"] <= 1.0
    _check(entries)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("inst", list(HI.ATT_INST))
@pytest.mark.parametrize("T", HI.ATT_SHORT + HI.ATT_LONG)
def test_attention_on_hard_softmax_rows(dev, T, inst):
    """Every softmax family on the short (T <= 32) and long kernels, forward and backward per input-type instance; dropout
    p = 0.1 on the peaked and rising families; on the long kernels the cliff family's rescale factor underflows to 0; bf16
    outputs are the round-to-nearest-even of the fp32 ones."""
    from tecmollm import ops, rng
    entries = []
    for fam in HI.SOFTMAX_FAMILIES:
        e, extras = HI.att_run(ops, rng, dev, fam, T, inst)
        assert all(extras.values()), (fam, extras)
        entries += e
    _check(entries)


# ------------------------------------------------------------------------------------------------ GATv2 neighbour softmax
@pytest.mark.parametrize("v2", [True, False], ids=["fwd2_bwd2", "fwd_bwd"])
@pytest.mark.parametrize("variation", HI.SPATIAL_VARIATIONS)
@pytest.mark.parametrize("graph", HI.SPATIAL_GRAPHS)
def test_spatial_stage_on_hard_logits(dev, graph, variation, v2, monkeypatch):
    """csrc/spatial_fwd2 + spatial_bwd2 (default) and spatial_fwd + spatial_bwd (TECM_SPATIAL_V2 = 0), with spatial_dx, on a
    peaked neighbour softmax, large leaky-ReLU arguments and large lin_l / lin_r biases: forward, the eleven parameter
    gradients and d x against the float64 oracle."""
    from tecmollm import functions as F_
    for var in ("TECM_SPATIAL_V2", "TECM_SPATIAL_BWD2"):
        monkeypatch.delenv(var, raising=False)
    if not v2:
        monkeypatch.setenv("TECM_SPATIAL_V2", "0")
    rec, real = [], F_.lib

    class Spy:
        def __getattr__(self, name):
            if name.startswith("tecm_spatial_") and "ws_floats" not in name:
                rec.append(name)
            return getattr(real(), name)
    monkeypatch.setattr(F_, "lib", lambda: Spy())
    entries, extras = HI.spatial_run(R, dev, graph, variation)
    want = {"tecm_spatial_fwd2", "tecm_spatial_bwd2"} if v2 else {"tecm_spatial_fwd", "tecm_spatial_bwd"}
    assert want <= set(rec) and "tecm_spatial_dx" in rec, rec
    assert all(extras.values()), extras
    assert len(entries) == 13
    _check(entries)


# ------------------------------------------------------------------------------------------------ activations
@pytest.mark.parametrize("name", [f.name for f in GC.FAMILIES])
def test_gelu_epilogues_on_the_value_grid(dev, name, monkeypatch):
    """tanh- and erf-GELU and their derivatives through every GEMM family's epilogue on 257 points of [-40, 40] and +-0,
    +-1e-30, +-1e-41: |act - ref| <= 1e-6 + 2^-22 |ref| (one bf16 ulp for a bf16 C), |act' - ref| <= 2e-6, all finite,
    act(x) == x from 10 up and |act(x)| <= 1e-6 from -10 down."""
    from tecmollm import ops
    fam = GC.FAMILY[name]
    for var in GC.ENV_SWITCHES:
        monkeypatch.delenv(var, raising=False)
    for var, val in fam.env.items():
        monkeypatch.setenv(var, val)
    fails = HI.act_sweep(ops, dev, fam, GC.ACT_GELU_ERF, GC.ACT_GELU_TANH)
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------ Huber
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
def test_huber_on_the_kink_and_at_the_extremes(dev, strided):
    from tecmollm import ops
    n = 4099
    e, tgt = HI.huber_errors(n)
    if strided:
        pred = e.view(1, n, 1).to(dev).permute(0, 2, 1).unsqueeze(-1)
        loss, dp = ops.huber_fwd_bwd_strided(pred, tgt.view(1, 1, n, 1).to(dev), 1.0, 1.0)
    else:
        loss, dp = ops.huber_fwd_bwd(e.to(dev), tgt.to(dev), 1.0, 1.0)
    dp = dp.reshape(-1).cpu()
    ed = e.double()
    ref = torch.where(ed.abs() <= 1, 0.5 * ed * ed, ed.abs() - 0.5).mean()
    g = ed.clamp(-1, 1) / n
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item()) + 1e-7
    assert bool(torch.isfinite(dp).all()) and bool(((dp.double() - g).abs() <= 2.0 ** -22 * g.abs()).all())
    # at and around the kink: every |e| >= 1 has the one saturated value, the neighbour below 1 is not above it, 0 gives 0
    sat = dp[e >= 1]
    assert bool((sat == sat[0]).all()) and bool((dp[e <= -1] == -sat[0]).all())
    below = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    assert bool((dp[e == below] <= sat[0]).all()) and bool((dp[e == below] > 0.999 * sat[0]).all())
    assert bool((dp[e == 0] == 0).all())


# ------------------------------------------------------------------------------------------------ fused clip + AdamW
@pytest.mark.parametrize("kind", ["zero", "tiny", "one_huge"])
def test_fused_clip_adamw_on_degenerate_gradients(dev, kind):
    """5 steps against torch (clip_grad_norm_ + AdamW): an all-zero gradient (norm 0: the update is the weight decay alone),
    gradients of 1e-30 (their squares underflow), one element of 1e18 among randn.  Bars of
    test_fused_clip_adamw_matches_torch."""
    from tecmollm.optim import CosineWarmRestarts, FlatAdamW
    shapes = [(257, 33), (33,), (65,)]
    g = torch.Generator().manual_seed(3)
    params0 = [torch.randn(*s, generator=g) for s in shapes]
    steps = 5
    if kind == "zero":
        grads = [[torch.zeros(*s) for s in shapes] for _ in range(steps)]
    elif kind == "tiny":
        grads = [[torch.full(s, 1e-30) * (1 - 2 * (torch.arange(int(np.prod(s))).view(s) % 2)) for s in shapes] for _ in range(steps)]
    else:
        grads = [[torch.randn(*s, generator=g) for s in shapes] for _ in range(steps)]
        for k in range(steps):
            grads[k][0][3 + k, 5] = 1e18
    want, norms, lrs = S.reference_optimizer_steps(params0, grads, lr=1e-3, weight_decay=1e-2, max_norm=1.0)
    ps = [torch.nn.Parameter(p.clone().to(dev)) for p in params0]
    opt = FlatAdamW(ps, lr=1e-3, weight_decay=1e-2)
    sched = CosineWarmRestarts(1e-3)
    for k in range(steps):
        for p, gk in zip(ps, grads[k]):
            p.grad.copy_(gk)
        tn = opt.step(lr=sched.lr, max_norm=1.0)
        assert abs(float(tn) - norms[k]) <= 2e-6 * norms[k], (k, float(tn), norms[k])
        sched.step()
    for p, w in zip(ps, want):
        assert bool(torch.isfinite(p).all())
        torch.testing.assert_close(p.detach().cpu(), w, rtol=2e-5, atol=2e-7)
    if kind == "zero":                                      # exactly the decoupled weight decay, step by step
        decayed = [p.clone() for p in params0]
        for k in range(steps):
            decayed = [d * (1 - lrs[k] * 1e-2) for d in decayed]
        for p, d in zip(ps, decayed):
            torch.testing.assert_close(p.detach().cpu(), d, rtol=3e-7, atol=0)
