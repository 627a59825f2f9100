"""GPU tests of the tiled spatial kernels at every tiling tecmollm/graph.py:build can choose (tests/spatial_tiling_cases.py; the
table is pinned by tests/test_host_spatial_tiling.py): through functions.SpatialFn, as TEC_MoLLM.forward runs the stage, against
the CPU oracle's embed + GATv2 + residual and autograd through it.

Per case, in both `graphs_with_edges` modes, in eval and in training mode (alpha dropout, the oracle given the mirrored masks):
the forward (columns 22, 23 exactly zero, everything finite), all eleven parameter gradients and d x, at the stage bar of
tests/parity.py (assert_close: RTOL in the max norm and the element-wise bar with ATOL_RMS, no kink allowance), and the entry
points that served the call.  Where the second formulation serves, the same call is made again with TECM_SPATIAL_V2=0 and compared
with the oracle as well, so that a case of at most 256 rows tests spatial_fwd2, spatial_bwd2, spatial_fwd and spatial_bwd<1>, and
a wider one spatial_fwd and spatial_bwd<2>.

With TECM_SPATIAL_TILING_LOG=<file> the module writes the worst rel_err / elem_err per case and kernel:
profiles/spatial_tiling_domain.txt is such a run."""
import os

import pytest
import torch

from tests import spatial_tiling_cases as sc
from tests.parity import assert_close, elem_err, rel_err

pytestmark = pytest.mark.gpu
ALL = [(c, cin) for case in sc.CASES for c, cin in sc.variants(case)]
_REC = {}                                                  # (case, Cin, kernel) -> [worst rel_err, worst elem_err, runs]
_meta = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield torch.device("cuda")
    path = os.environ.get("TECM_SPATIAL_TILING_LOG")
    if path:
        with open(path, "w", encoding="utf-8") as f:
            f.write("# case Cin (B, L) tiling = (tile_nodes, num_tiles, win_max, tile_edges_max) kernel: worst max-norm rel_err and "
                    "worst elem_err (fraction of the element-wise bar)\n# over both graph modes, eval and train, and the tensors "
                    "the kernel produces (forward: out; backward: eleven gradients; spatial_dx: d x)\n")
            for (name, cin, kern), (r, e, n) in _REC.items():
                c = sc.BY_NAME[name]
                f.write(f"{name:18s} cin={cin:<2d} B={c.B} L={c.L:<2d} tiling={str(c.tiling):22s} {kern:15s} "
                        f"rel_err={r:.2e} elem_err={e:.4f} runs={n}\n")


def _device_meta(c, cin, dev):
    from tecmollm import graph
    if (c.name, cin) not in _meta:
        _meta[(c.name, cin)] = graph.build(sc.edges(c), c.N, dev, 22 - cin)
    m = _meta[(c.name, cin)]
    assert (m.tile_nodes, m.num_tiles, m.win_max, m.tile_edges_max) == c.tiling
    return m


def _run(c, cin, mode, train, dev):
    """One forward + backward of the fused stage on the device: (out (B, L, N, 24), {"dx", every name of sc.SPATIAL})."""
    from tecmollm import functions as F_
    p, x, tf, gout = sc.stage_inputs(c, cin)
    meta = _device_meta(c, cin, dev)
    ps = [p[n].to(dev).requires_grad_(True) for n in sc.SPATIAL]
    tfd = tf[:, :, 0, :].contiguous().to(dev).unsqueeze(-2).expand(c.B, c.L, c.N, 4)
    plan = F_.DropPlan(True, 0.1, sc.DROP_SEED) if train else F_.DropPlan(False, 0.0, 0)
    xd = x.to(dev).requires_grad_(True)
    out = F_.SpatialFn.apply(xd, tfd, *ps, meta, 2, 1 if mode == "reference" else c.B * c.L, plan)
    gpad = torch.zeros(c.B, c.L, c.N, 24)
    gpad[..., :22] = gout
    grads = torch.autograd.grad(out, [xd] + ps, gpad.to(dev))
    torch.cuda.synchronize()
    return out.detach(), dict(zip(["dx"] + sc.SPATIAL, grads))


def _note(c, cin, kern, r, e):
    rec = _REC.setdefault((c.name, cin, kern), [0.0, 0.0, 0])
    rec[0], rec[1], rec[2] = max(rec[0], r), max(rec[1], e), rec[2] + 1


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("c,cin", ALL, ids=[f"{c.name}_cin{cin}" for c, cin in ALL])
def test_spatial_stage_matches_the_oracle_at_this_tiling(dev, c, cin, mode, train, monkeypatch):
    from tecmollm import functions as F_
    for var in ("TECM_SPATIAL_V2", "TECM_SPATIAL_BWD2"):
        monkeypatch.delenv(var, raising=False)
    rec = []
    real = F_.lib

    class Spy:                                              # which entry points served the call
        def __getattr__(self, name):
            if name in sc.ENTRY_POINTS:
                rec.append(name)
            return getattr(real(), name)
    monkeypatch.setattr(F_, "lib", lambda: Spy())
    want = sc.oracle(c, cin, mode, train)
    runs = [(True, [c.fwd, c.bwd])]
    if (c.fwd, c.bwd) != (sc.FWD1, sc.BWD1):                # the first formulation on the same call
        runs.append((False, [sc.FWD1, sc.BWD1]))
    failures = []
    for v2, route in runs:
        if not v2:
            monkeypatch.setenv("TECM_SPATIAL_V2", "0")
        rec.clear()
        out, got = _run(c, cin, mode, train, dev)
        assert rec == route, (rec, route)
        kf, kb = sc.kernels(c, v2)
        assert out.shape == (c.B, c.L, c.N, 24) and torch.isfinite(out).all()
        assert float(out[..., 22:].abs().max()) == 0.0
        for name, kern, a, b in [("out", kf, out[..., :22], want["out"]), ("dx", "spatial_dx", got["dx"], want["dx"])] + \
                                [(n, kb, got[n], want[n]) for n in sc.SPATIAL]:
            assert torch.isfinite(a).all(), (kern, name)
            r, e = rel_err(a, b), elem_err(a, b)
            print(f"{c.name} cin={cin} {mode} train={train} {kern} {name}: max-norm {r:.2e}, element-wise {e:.3f} of the bar")
            _note(c, cin, kern, r, e)
            try:
                assert_close(a, b, f"{kern} {name}")
            except AssertionError as err:
                failures.append(str(err))
    assert not failures, failures
    if train:                                               # the mask really is applied: the eval oracle is another result
        assert rel_err(want["out"], sc.oracle(c, cin, mode, False)["out"]) > 1e-3
