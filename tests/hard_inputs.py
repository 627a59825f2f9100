"""Hard-valued inputs for the norm, softmax and activation kernels (tests/test_gpu_hard_inputs.py,
tests/test_host_hard_inputs.py, tools/hard_inputs_report.py): deterministic input families away from N(0, 1), a
row-relative error metric, the plain fp32 CPU evaluation every kernel result is held against, and the bars.

Every value of every family is finite.  Nothing here needs a GPU: the kernel launchers take the `ops` module and a device.

A case yields entries (label, got_gpu, got_cpu32, ref64, row_dims): need_gpu = need(got_gpu, ref64), need_cpu =
need(got_cpu32, ref64), and the case passes when passes(need_gpu, need_cpu) (see BAR, K, FLOOR below)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

BAR = 1e-3                 # the project's parity bar
# K: smallest power of two >= twice the largest need_gpu / need_cpu measured on an MI355X over the cases that meet BAR;
# FLOOR: twice the largest need_gpu among the cases whose need_cpu is below EXACT.  Both as tools/hard_inputs_report.py
# derives them from the table in profiles/hard_inputs.txt.
K = 16.0
FLOOR = 5.69e-6
EXACT = 1e-6
EPS = 1e-5


# ------------------------------------------------------------------------------------------------ metric
def _rms(t, dims):
    if dims == ():                                   # a row of one element
        return t.abs()
    return t.pow(2).mean(dim=dims, keepdim=True).sqrt() if dims is not None else t.pow(2).mean().sqrt()


def need_map(got, ref, row_dims):
    """Per element: the smallest t with |got - ref| <= t * (|ref| + 0.1 * rms_row(ref) + 0.01 * rms_all(ref)); rms_row over
    `row_dims` (None: the whole tensor).  An element that is not finite needs inf; 0 / 0 is 0."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = ref.abs() + 0.1 * _rms(ref, row_dims) + 0.01 * _rms(ref, None)
    d = (got - ref).abs()
    t = torch.where(d == 0, torch.zeros_like(d), d / den)
    return torch.where(torch.isfinite(got), t, torch.full_like(t, float("inf")))


def need(got, ref, row_dims):
    return float(need_map(got, ref, row_dims).max())


def passes(need_gpu, need_cpu, k=None, floor=None):
    k, floor = K if k is None else k, FLOOR if floor is None else floor
    return need_gpu <= BAR and need_gpu <= max(k * need_cpu, floor)


def bar_in_force(need_cpu):
    return min(BAR, max(K * need_cpu, FLOOR))


def bf16_ok_scaled(got, ref, rms_row, rms_all):
    """bf16_ok with the row and tensor scales given (a strided subset of a group keeps the group's scale)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    lim = 2.0 ** -7 * ref.abs() + BAR * (0.1 * rms_row.double().cpu() + 0.01 * rms_all.double().cpu())
    r = torch.where(torch.isfinite(got), (got - ref).abs() / (lim + 1e-300), torch.full_like(ref, float("inf")))
    return float(r.max())


def bf16_ok(got, ref, row_dims):
    """A bf16 output against float64: one bf16 ulp of the value (2^-7 |ref|: half an ulp of rounding and as much again of
    arithmetic) plus the parity bar on the row's scale, BAR * (0.1 rms_row + 0.01 rms_all) -- the fp32 value in front of
    the rounding is held to no more than that.  Returns the worst ratio (<= 1 passes)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    lim = 2.0 ** -7 * ref.abs() + BAR * (0.1 * _rms(ref, row_dims) + 0.01 * _rms(ref, None))
    r = torch.where(torch.isfinite(got), (got - ref).abs() / (lim + 1e-300), torch.full_like(ref, float("inf")))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ norm families
NORM_FAMILIES = ("offset", "outlier_channels", "outlier_element", "tiny", "big", "constant", "onehot")
LN_OFFSET = 2e2            # the largest offsets at which plain fp32 stays under BAR / 4 (tests/test_host_hard_inputs.py)
GN_OFFSET = 1e2
# the constant family's value: 0.37 for LayerNorm; for GroupNorm, where fp32's rounding of the mean (times rstd = 316) is
# judged against gelu(beta) = O(0.05), plain fp32 needs 1.9e-4 .. 2.8e-4 at 0.37 (no margin under BAR / 4) and half that at 0.2
CONSTANT, GN_CONSTANT = 0.37, 0.2
OUTLIER_CHANNELS = ((5, 300.0), (100, -500.0), (200, 3000.0))


def norm_group(family, shape, seed, offset=LN_OFFSET, constant=CONSTANT):
    """One normalised group of `shape` (last dimension: channels) of the family."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(*shape, generator=g)
    C = shape[-1]
    if family == "randn":
        return x
    if family == "offset":
        return x + offset
    if family == "outlier_channels":
        for c, v in OUTLIER_CHANNELS:
            x[..., c % C] = v
        return x
    if family == "outlier_element":
        x.view(-1)[(7 * seed + 3) % x.numel()] = 2000.0
        return x
    if family == "tiny":
        return x * 1e-4
    if family == "big":
        return x * 1e4
    if family == "constant":
        return torch.full(shape, constant)
    if family == "onehot":
        x = x * 0.01
        x.view(-1)[(11 * seed + 5) % x.numel()] = 50.0
        return x
    raise ValueError(family)


def norm_rows(families, per, D, offset=LN_OFFSET, seed=0):
    """`per` consecutive rows of width D for each family of `families`: the `mixed` launch.  Returns (x (M, D), names)."""
    rows, names = [], []
    for i, fam in enumerate(families):
        for r in range(per):
            rows.append(norm_group(fam, (D,), seed + 31 * i + r, offset))
            names.append(fam)
    return torch.stack(rows), names


def gn_input(Bn, L, N, Cout, start, offset=GN_OFFSET, seed=0):
    """y (Bn, L, N, 3*Cout): sequence s = b*N + n is of family NORM_FAMILIES[(start + s) % 7] in all three branches; the
    branches of an `offset` sequence sit at (+c, -c/2, +c/4), as three conv biases would put them.  Returns (y, names)."""
    y = torch.empty(Bn, L, N, 3 * Cout)
    names = []
    for b in range(Bn):
        for n in range(N):
            s = b * N + n
            fam = NORM_FAMILIES[(start + s) % len(NORM_FAMILIES)]
            names.append(fam)
            for j, f in enumerate((1.0, -0.5, 0.25)):
                y[b, :, n, j * Cout:(j + 1) * Cout] = norm_group(fam, (L, Cout), seed + 97 * s + j, offset * f, GN_CONSTANT)
    return y, names


def affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_cpu(x, gamma, beta, dy, dtype):
    """(y, mean, rstd, dx, dgamma, dbeta) of LayerNorm over the last dimension in `dtype` on the CPU."""
    xd = x.to(dtype).requires_grad_(True)
    gd, bd = gamma.to(dtype).requires_grad_(True), beta.to(dtype).requires_grad_(True)
    y = F.layer_norm(xd, (x.shape[-1],), gd, bd, EPS)
    mean = xd.detach().mean(-1)
    rstd = 1.0 / torch.sqrt(xd.detach().var(-1, unbiased=False) + EPS)
    if dtype == torch.float32:                       # the statistics F.layer_norm itself forms in fp32
        _, mean, rstd = torch.native_layer_norm(xd.detach(), (x.shape[-1],), gd.detach(), bd.detach(), EPS)
        mean, rstd = mean.reshape(-1), rstd.reshape(-1)
    gx, gg, gb = torch.autograd.grad(y, (xd, gd, bd), dy.to(dtype))
    return y.detach(), mean, rstd, gx, gg, gb


def ln_entries(got, cpu, ref, tag=""):
    """got / cpu / ref: (y, mean, rstd, dx, dgamma, dbeta) tuples (None: not produced).  y and dx are judged on the
    normalised row, the statistics per row (rms_row = |ref|), the parameter gradients on the whole tensor."""
    out = []
    for i, (name, dims) in enumerate((("y", (-1,)), ("mean", ()), ("rstd", ()), ("dx", (-1,)), ("dgamma", None), ("dbeta", None))):
        if got[i] is not None:
            out.append((tag + name, got[i], cpu[i], ref[i], dims))
    return out


# ------------------------------------------------------------------------------------------------ GroupNorm(1) + GELU
def gn_cpu(y, gamma, beta, Cout, dact_full, dtype):
    """GroupNorm(1, Cout) + GELU per branch over the (L, Cout) group of every sequence of y (Bn, L, N, 3*Cout), in `dtype` on
    the CPU: (act, mean (S, 3), rstd (S, 3), dy, dgamma, dbeta, dysum) with dact_full the gradient of act (zeros where the
    strided consumer reads nothing)."""
    Bn, L, N, CT = y.shape
    yd = y.to(dtype).requires_grad_(True)
    gd, bd = gamma.to(dtype).requires_grad_(True), beta.to(dtype).requires_grad_(True)
    ys = yd.permute(0, 2, 3, 1).reshape(Bn * N, CT, L)
    outs, means, rstds = [], [], []
    for j in range(3):
        sl = slice(j * Cout, (j + 1) * Cout)
        outs.append(F.gelu(F.group_norm(ys[:, sl], 1, gd[sl], bd[sl], EPS)))
        grp = ys[:, sl].detach().reshape(Bn * N, -1)
        if dtype == torch.float32:
            _, m, r = torch.native_group_norm(ys[:, sl].detach().contiguous(), gd[sl].detach(), bd[sl].detach(), Bn * N, Cout, L, 1, EPS)
            m, r = m.reshape(-1), r.reshape(-1)
        else:
            m, r = grp.mean(-1), 1.0 / torch.sqrt(grp.var(-1, unbiased=False) + EPS)
        means.append(m)
        rstds.append(r)
    act = torch.cat(outs, 1).view(Bn, N, CT, L).permute(0, 3, 1, 2)
    gy, gg, gb = torch.autograd.grad(act, (yd, gd, bd), dact_full.to(dtype))
    return act.detach(), torch.stack(means, 1), torch.stack(rstds, 1), gy, gg, gb, gy.sum((0, 1, 2))


def gn_groups(t, Cout):
    """(Bn, L, N, 3*Cout) -> (Bn, L, N, 3, Cout): rms over dims (1, 4) is the (branch, sequence) group."""
    return t.reshape(*t.shape[:3], 3, Cout)


GN_ROW = (1, 4)


# ------------------------------------------------------------------------------------------------ softmax families
H, D = 12, 768
HD = D // H
SOFTMAX_FAMILIES = ("peaked3", "peaked8", "peaked16", "rising", "falling", "cliff", "sink", "common_offset", "uniform",
                    "identical_keys")
PEAKED_STD = {"peaked3": 3.0, "peaked8": 8.0, "peaked16": 16.0}
# Forward only: with logits of std 8 / 16 the BACKWARD of plain fp32 PyTorch needs 4e-4 .. 6e-4 (ds = p (dp - sum p dp) cancels
# on near one-hot rows, and the error reaches dq / dk multiplied by the scaled k / q), above the BAR / 4 the families are
# held to; std 3 is the largest scale whose backward stays under it (1.0e-4), so the backward is tested there.
FWD_ONLY = ("peaked8", "peaked16")
DROPPED = ("peaked3", "peaked8", "peaked16", "rising")           # dropout p = 0.1 on these only
# The rising family's largest logit (64: plain fp32 needs 4e-4 at T = 130; 32: 1.9e-4; 24: 1.5e-4).  Past 25 keys the slope
# is below 1 per key, and over a 16-key tile of the long kernels the running maximum moves by 3 (T = 130) or 1.15 (T = 333):
# every rescale factor alpha = exp(m - mn) is well below 1, none underflows.  The underflow is the cliff family's.
LOGIT_CAP = 24.0
# cliff: to the queries from 32 on, keys 0 .. 15 (the first 16-key tile of the long kernels) lie CLIFF below all later keys,
# so alpha = exp(-CLIFF) is exactly 0 in fp32 at their second tile; the earlier queries see plain logits.  No logit is large
# where it matters, so plain fp32 needs no more than on randn.
CLIFF, CLIFF_KEYS, CLIFF_QUERY = 120.0, 16, 32
COMMON_OFFSET = 16.0       # (25: plain fp32 needs 2.3e-4 at T = 333, no margin under BAR / 4)
SINK = 30.0
DROP_P, DROP_SEED = 0.1, 777


def softmax_qkv(family, Bn, T, N, seed=0):
    """qkv (Bn, T, N, 3*D) of the family.  q and k are 0.5 * randn with their component along u = (1, ..., 1) / 8 of every
    head removed; the constructed part lies along u: q carries 8 u (1 in every component), so a key that carries c u / 1
    (c / 8 in every component) shifts its logit by exactly c under the 1 / sqrt(64) scale."""
    g = torch.Generator().manual_seed(500 + 13 * T + seed)
    t = 0.5 * torch.randn(Bn, T, N, 3, H, HD, generator=g)
    q, k = t[:, :, :, 0], t[:, :, :, 1]                        # views (Bn, T, N, H, HD)
    j = torch.arange(T, dtype=torch.float32).view(1, T, 1, 1, 1)
    shift = None                                               # per-key logit shift, broadcast over (Bn, T, N, H, 1)
    along_u = 1.0                                              # the queries' component along 8 u (cliff: per query)
    if family in PEAKED_STD:                                   # logits of std 3 / 8 / 16: s^2 * 0.25 * sqrt(64) / 8
        s = math.sqrt(PEAKED_STD[family]) / 0.5
        q *= s
        k *= s
    elif family in ("rising", "falling"):
        slope = min(1.0, LOGIT_CAP / max(T - 1, 1))
        shift = (slope if family == "rising" else -slope) * j
    elif family == "cliff":
        a = math.sqrt(CLIFF / 8.0)                             # the product split evenly: q and k components of +-3.9, not 1 and 15
        shift = torch.where(j < CLIFF_KEYS, torch.tensor(-CLIFF / a), torch.tensor(0.0))
        along_u = a * (j >= CLIFF_QUERY).float()
    elif family == "sink":
        shift = torch.where(j == 0, torch.tensor(SINK), torch.tensor(0.0))
    elif family == "common_offset":
        shift = torch.full_like(j, COMMON_OFFSET)
    elif family == "uniform":
        q.zero_()
    elif family == "identical_keys":
        k[:] = k[:, :1].clone()
    elif family != "randn":
        raise ValueError(family)
    if shift is not None:
        q -= q.mean(-1, keepdim=True)
        k -= k.mean(-1, keepdim=True)
        q += along_u
        k += shift / 8.0
    return t.reshape(Bn, T, N, 3 * D)


def attention_ref(qkv, Bn, T, N, keep=None):
    """Causal multi-head attention in qkv's dtype (tests/test_gpu_ops.py::_ref_attention): (Bn, T, N, D)."""
    q, k, v = qkv.view(Bn, T, N, 3, H, HD).permute(3, 0, 2, 4, 1, 5)
    w = (q @ k.transpose(-1, -2)) / math.sqrt(HD)
    w = w.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool, device=qkv.device)), float("-inf")).softmax(-1)
    if keep is not None:
        w = w * keep
    return (w @ v).permute(0, 3, 1, 2, 4).reshape(Bn, T, N, D)


def attention_eval(q_in, d_in, Bn, T, N, keep, dtype, device, grad=True):
    """(ctx, dqkv or None) in `dtype` on `device` from the values the kernel reads."""
    qd = q_in.to(device=device, dtype=dtype).requires_grad_(grad)
    kp = None if keep is None else keep.to(device=device, dtype=dtype)
    ctx = attention_ref(qd, Bn, T, N, kp)
    if not grad:
        return ctx, None
    (g,) = torch.autograd.grad(ctx, qd, d_in.to(device=device, dtype=dtype))
    return ctx.detach(), g


def attention_keep(rng, Bn, T, N, p=DROP_P, seed=DROP_SEED):
    """The kernel's dropout multipliers, index (((b*N + n)*H + h)*T + i)*T + j, as a (Bn, N, H, T, T) double tensor."""
    idx = np.arange(Bn * N * H * T * T, dtype=np.uint64)
    return torch.from_numpy(rng.keep_mult(seed, idx, p)).double().view(Bn, N, H, T, T)


def att_heads(t):
    """(Bn, T, N, k*D) -> (..., k*H, HD): rms over the last dimension is the head-dim vector of one (sequence, head, token)."""
    return t.reshape(*t.shape[:3], -1, HD)


# ------------------------------------------------------------------------------------------------ activation grid
def act_grid(bf16=False):
    """257 points on [-40, 40] and +-0, +-1e-30, +-1e-41 (a denormal); bf16-representable where the kernel reads bf16."""
    g = torch.cat([torch.linspace(-40.0, 40.0, 257), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-41, -1e-41])])
    return g.bfloat16().float() if bf16 else g


def gelu_ref(x64, tanh):
    return F.gelu(x64, approximate="tanh" if tanh else "none")


def dgelu_ref(x64, tanh):
    x = x64.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(gelu_ref(x, tanh).sum(), x)
    return g


ACT_ABS, ACT_REL, DACT_ABS = 1e-6, 2.0 ** -22, 2e-6


# ------------------------------------------------------------------------------------------------ Huber
def huber_errors(n, seed=0):
    """Errors pred - target with the kink (exactly +-delta and its neighbours), zeros, denormal-square and huge values among
    randn; delta = 1.  Returns (pred, target) fp32 with pred - target exactly these errors (target = 0)."""
    g = torch.Generator().manual_seed(900 + seed)
    e = torch.randn(n, generator=g)
    one = np.float32(1.0)
    up, dn = float(np.nextafter(one, np.float32(2.0))), float(np.nextafter(one, np.float32(0.0)))
    special = [1.0, -1.0, up, -up, dn, -dn, 0.0, -0.0, 1e-30, -1e-30, 1e4, -1e4]
    for i, v in enumerate(special * 8):
        e[(i * 41 + 3) % n] = v
    return e, torch.zeros(n)


# ================================================================================================ kernel launches
# Each runner returns (entries, extras): entries as described at the top; extras: {name: value} for the bf16 outputs and the
# property checks that are not need-bars (worst ratios, <= 1 passes; flags).
NAN = float("nan")
LN_SHAPES = (("mixed768", 768, NORM_FAMILIES + ("randn",), 8), ("offset256", 256, ("offset",), 5),
             ("outlier1024", 1024, ("outlier_channels",), 5))
LN_BWD = ("plain", "add32", "add16", "dy16", "seq_major")
LN_SEQ = (1, 2, 32)        # (B, T, N) of the sequence-major gradient: M = 64


def ln_inputs(shape):
    _, Dn, fams, per = [s for s in LN_SHAPES if s[0] == shape][0]
    x, names = norm_rows(fams, per, Dn)
    gamma, beta = affine(Dn, 2)
    return x, names, gamma, beta


def ln_gradients(M, Dn, inst, rng):
    """(what the kernel is handed, keyword arguments without device tensors, dy as float64, dy as the fp32 the kernel forms)."""
    g = torch.Generator().manual_seed(77)
    du, dy2 = torch.randn(M, Dn, generator=g), 0.3 * torch.randn(M, Dn, generator=g)
    if inst == "plain":
        return du, {}, du.double(), du
    if inst == "dy16":
        return du.bfloat16(), {}, du.bfloat16().double(), du.bfloat16().float()
    if inst in ("add32", "add16"):
        dt = torch.float32 if inst == "add32" else torch.bfloat16
        du, dy2 = du.to(dt), dy2.to(dt)
        mult = torch.from_numpy(rng.keep_mult(4321, np.arange(M * Dn, dtype=np.uint64).reshape(M, Dn), 0.1))
        return du, {"add": (dy2, Dn, (0.1, 4321, Dn))}, du.double() + mult.double() * dy2.double(), du.float() + mult * dy2.float()
    if inst == "seq_major":
        B, T, N = LN_SEQ
        assert B * T * N == M
        dseq = du.bfloat16().view(B, N, T * Dn)
        tm = dseq.view(B, N, T, Dn).permute(0, 2, 1, 3).reshape(M, Dn)
        return dseq, {"dy_seq_major": (T, N, None)}, tm.double(), tm.float()
    raise ValueError(inst)


def ln_refs(shape, inst, rng):
    """(fp32 CPU, float64) result tuples of ln_cpu for the shape and backward instance."""
    x, _, gamma, beta = ln_inputs(shape)
    _, _, dy64, dy32 = ln_gradients(x.shape[0], x.shape[1], inst, rng)
    return ln_cpu(x, gamma, beta, dy32, torch.float32), ln_cpu(x, gamma, beta, dy64, torch.float64)


def ln_run(ops, rng, dev, shape, insts=("plain",)):
    """LayerNorm forward once and the backward per instance.  Returns (entries, extras, names)."""
    x, names, gamma, beta = ln_inputs(shape)
    M, Dn = x.shape
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    y, st = torch.full((M, Dn), NAN, device=dev), torch.full((M, 2), NAN, device=dev)
    ops.layernorm_fwd(xd, Dn, gd, bd, y, Dn, st, M, Dn)
    entries, extras = [], {}
    for k, inst in enumerate(insts):
        arg, kw, dy64, dy32 = ln_gradients(M, Dn, inst, rng)
        kw = dict(kw)
        if "add" in kw:
            t, ld, (p, seed, dld) = kw["add"]
            kw["add"] = (t.to(dev), ld, ops.drop(p, seed, dld))
        dx = torch.full((M, Dn), NAN, device=dev)
        dg, db = ops.layernorm_bwd(arg.to(dev), Dn, xd, Dn, gd, st, None, dx, M, Dn, **kw)
        cpu, ref = ln_refs(shape, inst, rng)
        fwd = (y, st[:, 0], st[:, 1]) if k == 0 else (None, None, None)
        entries += ln_entries(fwd + (dx, dg, db), cpu, ref, f"ln/{shape}/{inst}/")
        if k == 0 and "constant" in names:
            rows = [i for i, n in enumerate(names) if n == "constant"]
            extras["constant_y_vs_beta"] = need(y[rows], beta.expand(len(rows), Dn), (-1,))
            extras["constant_dx_finite"] = bool(torch.isfinite(dx[rows]).all())
    return entries, extras, names


# name (the family groupnorm.hip dispatches it to): ((Bn, L, N, Cout, stride), all-bf16 tensors, the family of sequence 0).
# Sequence s is of family NORM_FAMILIES[(start + s) % 7]; every start is chosen so that the launch holds an `offset`
# sequence (|mean| >> std: what a one-pass variance gets wrong) and a `constant` one (zero variance) -- with three
# sequences that is (constant, onehot, offset), start 5.  tests/test_host_hard_inputs.py asserts it.
GN_SHAPES = {
    "generic": ((2, 6, 3, 64, 1), False, 0),
    "reg4": ((2, 48, 5, 64, 2), False, 3),
    "reg8": ((1, 96, 3, 64, 2), False, 5),
    "cout256": ((1, 12, 3, 256, 2), False, 5),
    "y16_a": ((2, 48, 5, 64, 2), True, 1),
    "y16_b": ((1, 24, 9, 128, 2), True, 4),
    "y16_c": ((2, 16, 7, 64, 1), True, 2),
    "y16_d": ((1, 40, 3, 64, 2), True, 5),
    "y16_cout256": ((1, 12, 3, 256, 2), True, 5),
}


def gn_refs(name):
    """(fp32 CPU, float64) result tuples of gn_cpu, and the inputs (y, dact, gamma, beta, names) as fp32 tensors holding the
    values the kernel reads (bf16-representable for the all-bf16 kernels)."""
    (Bn, L, N, Cout, stride), all16, start = GN_SHAPES[name]
    CT = 3 * Cout
    y, names = gn_input(Bn, L, N, Cout, start)
    gamma, beta = affine(CT, 3)
    g = torch.Generator().manual_seed(4)
    dact = torch.randn(Bn, (L + stride - 1) // stride, N, CT, generator=g)
    if all16:
        y, dact = y.bfloat16().float(), dact.bfloat16().float()
    full = torch.zeros(Bn, L, N, CT)
    full[:, ::stride] = dact
    return (gn_cpu(y, gamma, beta, Cout, full, torch.float32), gn_cpu(y, gamma, beta, Cout, full, torch.float64),
            (y, dact, gamma, beta, names))


def gn_entries(got, cpu, ref, Cout, tag=""):
    """got / cpu / ref: (act, mean, rstd, dy, dgamma, dbeta, dysum) (None: not judged by a need-bar)."""
    out = []
    for i, (nm, dims) in enumerate((("act", GN_ROW), ("mean", ()), ("rstd", ()), ("dy", GN_ROW), ("dgamma", None), ("dbeta", None),
                                    ("dysum", None))):
        if got[i] is not None:
            f = (lambda t: gn_groups(t, Cout)) if dims == GN_ROW else (lambda t: t)
            out.append((tag + nm, f(got[i]), f(cpu[i]), f(ref[i]), dims))
    return out


def gn_run(ops, dev, name):
    (Bn, L, N, Cout, stride), all16, _ = GN_SHAPES[name]
    CT = 3 * Cout
    La = (L + stride - 1) // stride
    cpu, ref, (y, dact, gamma, beta, names) = gn_refs(name)
    if all16:
        assert ops.gn_y16_ok(L, N, Cout)
    else:
        assert ops.gn_reg_ok(L, N, Cout) == (name != "generic")
    gd, bd = gamma.to(dev), beta.to(dev)
    st = torch.full((Bn * N, 3, 2), NAN, device=dev)
    entries, extras = [], {}
    tag = f"gn/{name}/"
    if all16:
        yd = y.bfloat16().to(dev)
        act = torch.full((Bn, La, N, CT), NAN, device=dev, dtype=torch.bfloat16)
        ops.groupnorm_gelu_fwd(yd, gd, bd, act, st, Bn, L, N, Cout, act_stride=stride)
        dy = torch.full((Bn, L, N, CT), NAN, device=dev, dtype=torch.bfloat16)
        dg, db, dys = ops.groupnorm_gelu_bwd(dact.bfloat16().to(dev), stride, yd, gd, bd, st, dy, Bn, L, N, Cout)
        full_act = gn_groups(ref[0], Cout)
        lim_ref = full_act[:, ::stride]                  # the kept time steps, on the scale of their whole group
        extras["act_bf16"] = bf16_ok_scaled(gn_groups(act.float(), Cout), lim_ref, _rms(full_act, GN_ROW), _rms(full_act, None))
        extras["dy_bf16"] = bf16_ok(gn_groups(dy.float(), Cout), gn_groups(ref[3], Cout), GN_ROW)
        got = (None, st[..., 0], st[..., 1], None, dg, db, dys)
    else:
        yd = y.to(dev)
        act = torch.full((Bn, L, N, CT), NAN, device=dev)
        ops.groupnorm_gelu_fwd(yd, gd, bd, act, st, Bn, L, N, Cout)
        dy = torch.full((Bn, L, N, CT), NAN, device=dev)
        dg, db, dys = ops.groupnorm_gelu_bwd(dact.to(dev), stride, yd, gd, bd, st, dy, Bn, L, N, Cout)
        got = (act, st[..., 0], st[..., 1], dy, dg, db, dys)
    entries = gn_entries(got, cpu, ref, Cout, tag)
    return entries, extras, names


ATT_SHORT = (1, 3, 6, 12, 13, 24, 32)
ATT_LONG = (33, 65, 130, 333)
ATT_INST = {"f32": (False, False), "q16": (True, False), "q16_d16": (True, True)}
ATT_BN, ATT_N = 2, 3


def att_inputs(family, T, inst):
    q16, d16 = ATT_INST[inst]
    qkv = softmax_qkv(family, ATT_BN, T, ATT_N)
    g = torch.Generator().manual_seed(100 + T)
    dctx = torch.randn(ATT_BN, T, ATT_N, D, generator=g)
    return (qkv.bfloat16() if q16 else qkv), (dctx.bfloat16() if d16 else dctx)


def att_refs(family, T, inst, rng, ref_dev):
    """((ctx, dqkv) fp32 on the CPU, (ctx, dqkv) float64 on ref_dev) on the values the instance reads."""
    q_in, d_in = att_inputs(family, T, inst)
    keep = attention_keep(rng, ATT_BN, T, ATT_N) if family in DROPPED else None
    grad = family not in FWD_ONLY
    return (attention_eval(q_in, d_in, ATT_BN, T, ATT_N, keep, torch.float32, "cpu", grad),
            attention_eval(q_in, d_in, ATT_BN, T, ATT_N, keep, torch.float64, ref_dev, grad))


def att_run(ops, rng, dev, family, T, inst):
    """Forward (once per forward instance) and backward of one family at one length.  The float64 reference runs on `dev` on
    the values the kernel reads, the fp32 comparator on the CPU."""
    if family in FWD_ONLY and ATT_INST[inst][1]:
        return [], {}
    q_in, d_in = att_inputs(family, T, inst)
    Bn, N = ATT_BN, ATT_N
    drop = ops.drop(DROP_P, DROP_SEED, 1) if family in DROPPED else None
    (cpu_ctx, cpu_g), (ref_ctx, ref_g) = att_refs(family, T, inst, rng, dev)
    qd, dd = q_in.to(dev), d_in.to(dev)
    entries, extras = [], {}
    tag = f"att/{family}/T{T}/{inst}/"
    if not ATT_INST[inst][1]:
        ctx = torch.full(ref_ctx.shape, NAN, device=dev)
        ops.attention_fwd(qd, ctx, Bn, T, N, H, D, drop)
        entries.append((tag + "ctx", att_heads(ctx), att_heads(cpu_ctx), att_heads(ref_ctx), (-1,)))
        ctx16 = torch.full(ref_ctx.shape, NAN, device=dev, dtype=torch.bfloat16)
        ops.attention_fwd(qd, ctx16, Bn, T, N, H, D, drop)
        extras["ctx16_is_rne"] = torch.equal(ctx16, ctx.bfloat16())
    if family in FWD_ONLY:
        return entries, extras
    dq = torch.full(q_in.shape, NAN, device=dev)
    ops.attention_bwd(qd, dd, dq, Bn, T, N, H, D, drop)
    entries.append((tag + "dqkv", att_heads(dq), att_heads(cpu_g), att_heads(ref_g), (-1,)))
    dq16 = torch.full(q_in.shape, NAN, device=dev, dtype=torch.bfloat16)
    ops.attention_bwd(qd, dd, dq16, Bn, T, N, H, D, drop)
    extras["dqkv16_is_rne"] = torch.equal(dq16, dq.bfloat16())
    return entries, extras


def measure(entries):
    """[(label, need_cpu, need_gpu)]"""
    return [(lab, need(cpu, ref, dims), need(got, ref, dims)) for lab, got, cpu, ref, dims in entries]


def failures(rows):
    return [f"{lab}: need_gpu {ng:.3g} need_cpu {nc:.3g} bar {bar_in_force(nc):.3g}" for lab, nc, ng in rows if not passes(ng, nc)]


# ------------------------------------------------------------------------------------------------ conv forward statistics
CONV_SHAPE = (2, 48, 7, 22, 24, 64)      # (Bn, Lc, N, cin, ld_in, Cout)
CONV_BIAS = 50.0
CONV_ACT_STRIDE = 2


def conv_stats_run(ops, rng, dev):
    """TecmConvFwd.stats on a y with |mean| >> std: branch biases of (+50, -50, +50) and inputs with a per-channel offset.
    (mean, rstd) against float64 statistics of the rounded y the kernel wrote; comparator: fp32 group_norm of that y.  Then
    the elementwise GroupNorm + GELU forward with these statistics given: its bf16 act against float64 (bf16_ok_scaled)."""
    Bn, Lc, N, cin, ld_in, Cout = CONV_SHAPE
    CT = 3 * Cout
    g = torch.Generator().manual_seed(31)
    inp = torch.zeros(Bn, Lc, N, ld_in)
    inp[..., :cin] = torch.randn(Bn, Lc, N, cin, generator=g) + torch.randn(cin, generator=g)
    ws = [0.2 * torch.randn(Cout, cin, k, generator=g) for k in (3, 5, 7)]
    bias = 0.1 * torch.randn(CT, generator=g) + torch.tensor([CONV_BIAS, -CONV_BIAS, CONV_BIAS]).repeat_interleave(Cout)
    y = torch.full((Bn, Lc, N, CT), NAN, device=dev, dtype=torch.bfloat16)
    stats = torch.full((Bn * N, 3, 2), NAN, device=dev)
    ops.conv_fwd(inp.bfloat16().to(dev), *[w.to(dev) for w in ws], bias.to(dev), y, Bn, Lc, N, Cout, cin, ld_in, stats=stats)
    yc = y.float().cpu().view(Bn, Lc, N, 3, Cout).permute(0, 2, 3, 1, 4).reshape(Bn * N * 3, Lc * Cout)
    assert bool(torch.isfinite(yc).all())
    yd = yc.double()
    mean, rstd = yd.mean(-1), 1.0 / torch.sqrt(yd.var(-1, unbiased=False) + EPS)
    ratio = float((mean.abs() * rstd).min())
    one = torch.ones(1)
    _, m32, r32 = torch.native_group_norm(yc.view(Bn * N * 3, 1, Lc * Cout), one, 0 * one, Bn * N * 3, 1, Lc * Cout, 1, EPS)
    st = stats.view(-1, 2)
    # the elementwise forward that takes these statistics as given (gn_apply_fwd16), on the time steps a stride-2 consumer keeps
    gamma, beta = affine(CT, 3)
    La = (Lc + CONV_ACT_STRIDE - 1) // CONV_ACT_STRIDE
    act = torch.full((Bn, La, N, CT), NAN, device=dev, dtype=torch.bfloat16)
    ops.groupnorm_gelu_fwd(y, gamma.to(dev), beta.to(dev), act, stats, Bn, Lc, N, Cout, act_stride=CONV_ACT_STRIDE, stats_given=True)
    xh = ((yd - mean[:, None]) * rstd[:, None]).view(Bn, N, 3, Lc, Cout).permute(0, 3, 1, 2, 4).reshape(Bn, Lc, N, CT)
    full_act = gn_groups(F.gelu(xh * gamma.double() + beta.double()), Cout)
    act_ok = bf16_ok_scaled(gn_groups(act.float(), Cout), full_act[:, ::CONV_ACT_STRIDE], _rms(full_act, GN_ROW), _rms(full_act, None))
    return ([("conv_stats/mean", st[:, 0], m32.reshape(-1), mean, ()), ("conv_stats/rstd", st[:, 1], r32.reshape(-1), rstd, ())],
            {"conv_stats/min |mean| / std": ratio, "conv_stats/act_bf16": act_ok})


# ------------------------------------------------------------------------------------------------ GATv2 neighbour softmax
SPATIAL_VARIATIONS = ("att16", "xoff", "bias30")
X_OFFSET = 30.0            # + 50: the fp32 oracle needs 3.7e-2 for d lin_r.weight on the grid (a gradient that cancels); + 30: 1e-4
SPATIAL_GRAPHS = ("grid", "hub")
SP_B, SP_L = 2, 3


# The kernels evaluate the neighbour softmax's backward in its closed form, de = alpha (dalpha - sum alpha dalpha).  The
# gradients of lin_r and att are sums of de over a target's sources that cancel (exactly, where the leaky-ReLU slope is the
# same for all of them): gat_closed_form is that form in plain PyTorch, the planted fault of tests/test_host_hard_inputs.py.
def gat_closed_form(R, p, x, tf, ei, gout, dtype, mode):
    """(d lin_r.bias, d lin_r.weight) of the stage from the closed-form softmax backward in `dtype`, every graph with its
    edges.  mode "plain": dalpha = <d out[i], x_l[j]> as it is; "shift": minus the self loop's <d out[i], x_l[i]>, which
    changes nothing in exact arithmetic (csrc/spatial_bwd.hip, B1)."""
    N = x.shape[2]
    pp = {k: v.to(dtype) for k, v in p.items()}
    h = R.embed(x.to(dtype), tf, pp).permute(1, 0, 2, 3).reshape(-1, 22)
    M = h.shape[0]
    Wl, bl, Wr, br = [pp[R.P_GAT + n] for n in ("lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias")]
    att = pp[R.P_GAT + "att"].view(1, 2, -1)
    xl, xr = (h @ Wl.t() + bl).view(M, 2, -1), (h @ Wr.t() + br).view(M, 2, -1)
    e2 = R.batched_edge_index(ei, N, M // N)
    keep = e2[0] != e2[1]
    loops = torch.arange(M)
    src, dst = torch.cat([e2[0][keep], loops]), torch.cat([e2[1][keep], loops])
    s = xl[src] + xr[dst]
    e = (F.leaky_relu(s, R.GAT_NEG_SLOPE) * att).sum(-1)
    emax = torch.full((M, 2), float("-inf"), dtype=dtype).scatter_reduce(0, dst.view(-1, 1).expand(-1, 2), e, reduce="amax")
    pe = (e - emax[dst]).exp()
    alpha = pe / torch.zeros(M, 2, dtype=dtype).index_add_(0, dst, pe)[dst]
    gv = gout.to(dtype).permute(1, 0, 2, 3).reshape(M, 2, -1)
    da = (gv[dst] * xl[src]).sum(-1)
    if mode == "shift":
        da = da - (gv[dst] * xl[dst]).sum(-1)
    dot = torch.zeros(M, 2, dtype=dtype).index_add_(0, dst, alpha * da)
    de = alpha * (da - dot[dst])
    k = torch.where(s > 0, att.expand_as(s), R.GAT_NEG_SLOPE * att.expand_as(s))
    dxr = torch.zeros(M, 2, xl.shape[-1], dtype=dtype).index_add_(0, dst, de.unsqueeze(-1) * k).reshape(M, -1)
    return dxr.sum(0), dxr.t() @ h


def spatial_names(R):
    return [R.P_EMB + f"{n}_embedding.weight" for n in ("node", "tod", "doy", "year", "season")] + \
           [R.P_GAT + n for n in ("lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "att", "bias")]


def spatial_inputs(R, graph, variation):
    """(p, x, tf, ei, gout): the stage's parameters and inputs with the attention vector x 16 (peaked neighbour softmax), every
    input channel + X_OFFSET (large leaky-ReLU arguments) or lin_l / lin_r biases of +-30 (alternating by channel, so that the
    two do not cancel in xl[j] + xr[i])."""
    if graph == "grid":
        N = 135
        ei = R.grid_graph(9, 15, threshold_km=150.0)[0]
    else:                                                   # the hub multigraph of test_spatial_irregular_graphs
        N = 150
        g = torch.Generator().manual_seed(10)
        src, dst = torch.randint(0, N, (400,), generator=g), torch.randint(0, N, (400,), generator=g)
        dst[dst == 7] = 8
        hub = torch.stack([torch.arange(40, 100), torch.full((60,), 3)])
        loops = torch.stack([torch.arange(0, 20), torch.arange(0, 20)])
        ei = torch.cat([torch.stack([src, dst]), hub, loops, torch.stack([src[:50], dst[:50]])], 1)
    cfg = R.default_config(num_nodes=N)
    p = {k: v.clone() for k, v in R.init_params(cfg, seed=8).items() if k.startswith((R.P_EMB, R.P_GAT))}
    x, tf, _ = R.synthetic_batch(SP_B, SP_L, N, cfg["spatial_in_channels_base"], 12, seed=9)
    if variation == "att16":
        p[R.P_GAT + "att"] = p[R.P_GAT + "att"] * 16
    elif variation == "xoff":
        x = x + X_OFFSET
    elif variation == "bias30":
        n = p[R.P_GAT + "lin_l.bias"].numel()
        c = torch.arange(n)
        p[R.P_GAT + "lin_l.bias"] = 30.0 * (1 - 2 * (c % 2)).float()
        p[R.P_GAT + "lin_r.bias"] = 30.0 * (1 - 2 * ((c // 2) % 2)).float()
    else:
        raise ValueError(variation)
    gout = torch.randn(SP_B, SP_L, N, 22, generator=torch.Generator().manual_seed(11))
    return p, x, tf, ei, gout


def spatial_oracle(R, p, x, tf, ei, gout, dtype):
    """(out (B, L, N, 22), the eleven parameter gradients, d x) of the oracle's embed + GATv2 + residual in `dtype`, every
    graph with its edges.  On one thread: autograd's scatter-adds then run in a fixed order, and the fp32 result -- the
    comparator of the GPU bars -- is one value, not a range that depends on the machine's thread count."""
    B, L, N, _ = x.shape
    pr = {k: v.to(dtype).requires_grad_(True) for k, v in p.items()}
    xr = x.to(dtype).requires_grad_(True)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = R.spatial(R.embed(xr, tf, pr), ei, pr, 2, None).view(L, B, N, 22).permute(1, 0, 2, 3)
        assert out.dtype == dtype
        grads = torch.autograd.grad(out, [pr[n] for n in spatial_names(R)] + [xr], gout.to(dtype))
    finally:
        torch.set_num_threads(threads)
    return out.detach(), list(grads[:-1]), grads[-1]


def spatial_run(R, dev, graph, variation, tag=""):
    """The fused stage on the device (which kernels serve it is the caller's choice of TECM_SPATIAL_V2 / TECM_SPATIAL_BWD2)
    against the float64 oracle; comparator: the fp32 oracle."""
    from tecmollm import functions as F_
    from tecmollm import graph as G_
    p, x, tf, ei, gout = spatial_inputs(R, graph, variation)
    names = spatial_names(R)
    B, L, N, _ = x.shape
    cpu, ref = spatial_oracle(R, p, x, tf, ei, gout, torch.float32), spatial_oracle(R, p, x, tf, ei, gout, torch.float64)
    meta = G_.get(ei.to(dev), N, dev, p[names[0]].shape[1])
    ps = [p[n].to(dev).requires_grad_(True) for n in names]
    tfd = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(B, L, N, 4)
    xd = x.to(dev).requires_grad_(True)
    out = F_.SpatialFn.apply(xd, tfd, *ps, meta, 2, B * L, F_.DropPlan(False, 0.0, 0))
    gpad = torch.zeros(B, L, N, 24)
    gpad[..., :22] = gout
    grads = torch.autograd.grad(out, ps + [xd], gpad.to(dev))
    tag = f"spatial/{graph}/{variation}/{tag}"
    entries = [(tag + "out", out[..., :22].detach(), cpu[0], ref[0], (-1,))]
    for n, a, c, r in zip(names, grads[:-1], cpu[1], ref[1]):
        entries.append((tag + n.split(".", 1)[1], a, c, r, None))
    entries.append((tag + "dx", grads[-1], cpu[2], ref[2], (-1,)))
    return entries, {tag + "pad_columns_zero": float(out[..., 22:].detach().abs().max()) == 0.0}


# ------------------------------------------------------------------------------------------------ activation sweep
def act_sweep(ops, dev, fam, ACT_ERF, ACT_TANH):
    """The GEMM epilogues of one family of tests/gemm_epilogue_cases.py on a prescribed product: A holds one-hot rows
    (row m selects component m % R), B holds the grid in those R components, so C[m][n] = grid[(m % R) * N + n] exactly
    (padded with zeros).  Bias-free tanh- and erf-GELU with the pre-activation written, a bf16 C where the family has one
    (tanh only: the library refuses erf-GELU with a bf16 C, tests/gemm_epilogue_cases.py),
    and act'(grid) through dact_src on a product of ones.  Returns the list of failures (the family's environment
    switches are the caller's to set)."""
    M, N, Kd = fam.M, fam.N, fam.K
    grid = act_grid(fam.prec == 1)
    R_ = -(-grid.numel() // N)
    assert R_ <= M and R_ <= Kd
    Bm = torch.zeros(N, Kd)
    flat = torch.zeros(R_ * N)
    flat[:grid.numel()] = grid
    Bm[:, :R_] = flat.view(R_, N).t()
    A = torch.zeros(M, Kd)
    A[torch.arange(M), torch.arange(M) % R_] = 1.0
    want = flat.view(R_, N)[torch.arange(M) % R_]                      # (M, N): the product
    odt = torch.bfloat16 if fam.op16 else torch.float32

    def dev_ops(A_, B_):
        if fam.km:
            lda = fam.lda or M
            a = torch.zeros(Kd, lda)
            a[:, :M] = A_.t()
        else:
            lda, a = Kd, A_
        ldb, b = (N, B_.t().contiguous()) if fam.kn else (Kd, B_)
        return a.to(odt).to(dev), lda, b.to(odt).to(dev), ldb
    kw = dict(bf16=fam.prec, a_layout=ops.A_KM if fam.km else ops.A_MK, b_layout=ops.B_KN if fam.kn else ops.B_NK)
    a, lda, b, ldb = dev_ops(A, Bm)
    x64 = want.double()
    fails = []
    big, neg = want >= 10, want <= -10
    for name, act, tanh in (("tanh", ACT_TANH, True), ("erf", ACT_ERF, False)):
        ref = gelu_ref(x64, tanh)
        for c16 in ((False, True) if fam.prec == 1 and tanh else (False,)):
            C = torch.full((M, N), NAN, device=dev, dtype=torch.bfloat16 if c16 else torch.float32)
            pre = torch.full((M, N), NAN, device=dev)
            ops.gemm(M, N, Kd, a, lda, b, ldb, C, N, act=act, preact=(pre, N), **kw)
            got, gp = C.float().cpu(), pre.cpu()
            tag = f"{fam.name}/{name}{'/c16' if c16 else ''}"
            if not bool(torch.isfinite(got).all() and torch.isfinite(gp).all()):
                fails.append(f"{tag}: not finite")
                continue
            if not torch.equal(gp, want) and not bool(((gp.double() - x64).abs() <= ACT_ABS + ACT_REL * x64.abs()).all()):
                fails.append(f"{tag}: pre-activation off by {float((gp.double() - x64).abs().max()):.3g}")
            err = (got.double() - ref).abs()
            lim = 2.0 ** -7 * ref.abs() + 1e-6 if c16 else ACT_ABS + ACT_REL * ref.abs()
            if not bool((err <= lim).all()):
                i = int((err / lim).argmax())
                fails.append(f"{tag}: act({float(want.view(-1)[i])}) off by {float(err.view(-1)[i]):.3g} (bar {float(lim.view(-1)[i]):.3g})")
            if not torch.equal(got[big], want[big]):                        # (a bf16 C: the grid is bf16-representable)
                fails.append(f"{tag}: act(x) != x for x >= 10")
            if not float(got[neg].abs().max()) <= 1e-6:
                fails.append(f"{tag}: |act(x)| > 1e-6 for x <= -10")
    a1, lda1, b1, ldb1 = dev_ops((torch.arange(Kd) == 0).float().expand(M, Kd).contiguous(), (torch.arange(Kd) == 0).float().expand(N, Kd).contiguous())
    src = want.to(dev).contiguous()
    for name, act, tanh in (("tanh", ACT_TANH, True), ("erf", ACT_ERF, False)):
        Dm = torch.full((M, N), NAN, device=dev)
        ops.gemm(M, N, Kd, a1, lda1, b1, ldb1, Dm, N, act=act, dact_src=(src, N), **kw)
        err = (Dm.double().cpu() - dgelu_ref(x64, tanh)).abs()
        if not bool(torch.isfinite(Dm).all()):
            fails.append(f"{fam.name}/d{name}: not finite")
        elif not bool((err <= DACT_ABS).all()):
            i = int(err.argmax())
            fails.append(f"{fam.name}/d{name}: act'({float(want.view(-1)[i])}) off by {float(err.max()):.3g}")
    return fails
