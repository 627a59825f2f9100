"""Cost of the field scores (FieldMetrics / tecm_field_scores) at the full grid: N = 2911, K = 16 members, B = 16, L_out = 12,
8 distance classes, order 0.5.  Recorded, not gated.

  * kernel times of the five kernels of one update: a run of its own under `rocprofv3 --kernel-trace --stats` (a child process
    started before this one touches the GPU), read from the trace database, first update dropped.  Members node-contiguous
    (what `ensemble_members` returns), the dataset's target layout, one group, no per-sample outputs;
  * the same scores written with torch on the device (float64 norms; the pair terms in float32 and their sums in float64,
    256 rows of the class matrix and 16 maps at a time so that the (16, 256, N) temporaries fit, the class sums as one
    matrix product per chunk -- no host synchronisation inside), wall time around a synchronise, and the largest relative
    difference of its sums from the kernels';
  * wall time of `evaluate_ensemble` over two batches with and without `fields`, and of the K no-grad forwards of one batch
    (`ensemble_members`), each ending in a device synchronise, median of `--passes` alternating passes after one warm-up.

    python tools/fields_bench.py [--out PREFIX] [--no-profile]           # writes PREFIX.json and PREFIX.txt
"""
import argparse
import glob
import json
import os
import re
import sqlite3
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tec-mollm_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

from baseline_bench import CH, H, L_OUT, N, W, wall  # noqa: E402

B, K, L_IN = 16, 16, 48
EDGES_KM = (0.0, 150.0, 300.0, 600.0, 1000.0, 1500.0, 2500.0, 4000.0, float("inf"))
NB = len(EDGES_KM) - 1
PROFILE_UPDATES = 5
SCALER = (20.0, 8.0)
KERNELS = ("field_energy_kernel", "field_energy_sample_kernel", "field_pairs_kernel", "field_pairs_sample_kernel",
           "field_cells_kernel")


def classes():
    from tecmollm.fields import grid_pair_classes
    return grid_pair_classes(-10.0 + 1.0 * np.arange(H), 60.0 + 1.0 * np.arange(W), EDGES_KM)


def kernels_only():
    """The child run under the profiler: one warm-up update and PROFILE_UPDATES more."""
    import torch
    from src.evaluation.metrics import FieldMetrics
    torch.manual_seed(0)
    y = torch.randn(B, L_OUT, N, 1, device="cuda")
    mem = torch.randn(K, B, L_OUT, N, device="cuda")
    fm = FieldMetrics(L_OUT, N, K, torch.from_numpy(classes()), NB, 0.5, 1, SCALER)
    for _ in range(1 + PROFILE_UPDATES):
        fm.update(mem, y)
    torch.cuda.synchronize()


def profile_kernels(timeout=420):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "fields", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, start, end from kernels order by start").fetchall()
    out = {}
    for kern in KERNELS:
        us = [(e - s) / 1e3 for name, s, e in rows if re.search(kern + r"(?![a-z_])", name)]     # mangled or demangled
        if len(us) != 1 + PROFILE_UPDATES:
            raise RuntimeError(f"expected {1 + PROFILE_UPDATES} launches of {kern}, saw {len(us)}")
        u = us[1:]
        out[kern] = dict(launches=len(u), us=float(np.mean(u)), us_min=float(np.min(u)), us_max=float(np.max(u)))
    return out


def torch_scores(mem, y, pc, chunk=256, maps=16):
    """[sum A, sum D, sum E] and (NB, 3) [sum e^2, sum v_o, sum v_e] over every (sample, horizon), with torch on the device."""
    import torch
    from src.evaluation.metrics import TEC_MAX, TEC_MIN
    mean, scale = SCALER
    x = torch.nan_to_num(mem * scale + mean, nan=0.0, posinf=100.0, neginf=0.0).clamp_(TEC_MIN, TEC_MAX)      # (K, S, H, N)
    t = torch.nan_to_num(y.squeeze(-1) * scale + mean, nan=0.0, posinf=100.0, neginf=0.0)
    xd, td = x.double(), t.double()
    A = (xd - td).pow(2).sum(-1).sqrt().sum() / K
    D = torch.zeros((), device=x.device, dtype=torch.float64)
    for k in range(K - 1):
        D += (xd[k + 1:] - xd[k]).pow(2).sum(-1).sqrt().sum()
    E = (xd.mean(0) - td).pow(2).sum(-1).sqrt().sum()
    vs = torch.zeros(NB, 3, device=x.device, dtype=torch.float64)
    xf = x.reshape(K, -1, N)
    tf = t.reshape(-1, N)
    ids = torch.arange(NB, device=x.device, dtype=torch.uint8)
    for i0 in range(0, N, chunk):
        i1 = min(i0 + chunk, N)
        onehot = (pc[i0:i1].reshape(-1, 1) == ids).double()               # (c * N, NB): the class sums are one matmul, no sync
        for m0 in range(0, tf.shape[0], maps):
            tt, xx = tf[m0:m0 + maps], xf[:, m0:m0 + maps]
            vo = (tt[:, i0:i1, None] - tt[:, None, :]).abs().sqrt()                                      # (maps, c, N)
            ve = torch.zeros_like(vo)
            for k in range(K):
                ve += (xx[k, :, i0:i1, None] - xx[k, :, None, :]).abs().sqrt()
            ve /= K
            vod, ved = vo.double().reshape(vo.shape[0], -1), ve.double().reshape(vo.shape[0], -1)
            e = vod - ved
            vs += torch.stack([(e * e) @ onehot, vod @ onehot, ved @ onehot]).sum(1).T
    return torch.stack([A, D, E]), vs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (kernel times: not measured)")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    kern = {} if a.no_profile else profile_kernels()                       # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fields_bench.py measures on the GPU; none found")
    from oracle import ref_cpu as R
    from src.data.dataset import SlidingWindowSamplerDataset
    from src.evaluation.metrics import FieldMetrics
    from src.model.tec_mollm import TEC_MoLLM
    from tecmollm import ensemble_members, evaluate_ensemble, ops
    from tecmollm.fields import FieldSpec
    dev_name = torch.cuda.get_device_name(0)
    lines = [f"# {dev_name}; N = {N}, K = {K}, B = {B}, L_out = {L_OUT}, {NB} classes {EDGES_KM} km, order 0.5; "
             f"python tools/fields_bench.py" + (" --no-profile" if a.no_profile else "") + f" --passes {a.passes}"]

    def say(s):
        lines.append(s)
        print(s, flush=True)
    T, lds, ws = ops.field_scores_plan(B, L_OUT, N, K, NB)
    nt = -(-N // T)
    pairs = N * (N - 1) // 2
    terms = B * L_OUT * pairs * (K + 1)
    say(f"plan: node tile {T}, {nt * (nt + 1) // 2} tile pairs x {L_OUT} x {B} blocks of 256 threads, {lds} B of LDS, workspace "
        f"{ws / 1e6:.1f} MB; {pairs} pairs per map, {terms:.3e} pair terms per update")
    total_us = 0.0
    for name in KERNELS:
        if name in kern:
            k = kern[name]
            total_us += k["us"]
            say(f"{name}: {k['us']:.1f} us (min {k['us_min']:.1f}, max {k['us_max']:.1f}; rocprofv3 kernel trace, {k['launches']} launches)")
    if kern:
        pk = kern["field_pairs_kernel"]["us"]
        say(f"one update, five kernels: {total_us / 1e3:.3f} ms; pair kernel {terms / pk / 1e6:.2f} T pair terms/s")
    else:
        say("kernel times: not measured")
    # the same scores with torch
    torch.manual_seed(0)
    pc_np = classes()
    pc = torch.from_numpy(pc_np).cuda()
    y = torch.randn(B, L_OUT, N, 1, device="cuda")
    mem = torch.randn(K, B, L_OUT, N, device="cuda")
    fm = FieldMetrics(L_OUT, N, K, pc, NB, 0.5, 1, SCALER)
    fm.update(mem, y)
    ours = [wall(lambda: fm.update(mem, y)) for _ in range(a.passes)]
    fm.reset()
    fm.update(mem, y)
    es_k = fm.es_stats[0].sum(0)[1:]
    vs_k = fm.vs_stats[0].sum(0)[:, 2:]
    torch_scores(mem[:, :1, :1], y[:1, :1], pc)                            # warm-up on one map
    res = {}
    tt = wall(lambda: res.update(out=torch_scores(mem, y, pc)))
    es_t, vs_t = res["out"]
    rel_es = float(((es_t - es_k).abs() / es_k.abs()).max())
    rel_vs = float(((vs_t - vs_k).abs() / vs_k.abs().clamp_min(1e-300)).max())
    u = sorted(ours)[len(ours) // 2]
    say(f"FieldMetrics.update wall {u * 1e3:.2f} ms (host clock around a synchronise); the same sums with torch, 256 class rows x "
        f"16 maps at a time: {tt * 1e3:.0f} ms = {tt / u:.0f} x; largest relative difference of the sums: energy {rel_es:.2e}, "
        f"variogram {rel_vs:.2e}")
    del mem, y, fm, res
    # evaluate_ensemble with and without the field scores, two batches
    cfg = R.default_config(L_in=L_IN, L_out=L_OUT, num_nodes=N)
    torch.manual_seed(3)
    with torch.device("cuda"):
        model = TEC_MoLLM(dict(cfg, include_wte=False, load_pretrained_gpt2=False)).eval()
    Tt = L_IN + L_OUT + 2 * B - 1
    rng = np.random.default_rng(0)
    X = rng.standard_normal((Tt, H, W, CH), dtype=np.float32)
    t = np.arange(Tt)
    TF = np.stack([t % 12, t % 366, np.zeros(Tt), (t // 30) % 4], 1).astype(np.float32)
    Y = torch.zeros(Tt, H, W, L_OUT)
    Y[..., :] = torch.from_numpy(X[..., 0:1])
    ds = SlidingWindowSamplerDataset.from_tensors(torch.from_numpy(X), Y, torch.from_numpy(TF), L_IN, L_OUT, device="cuda", mode="test")
    assert len(ds) == 2 * B
    ei = R.grid_graph()[0].cuda()
    spec = FieldSpec(pc_np, EDGES_KM, 0.5)
    xb, tfb, _ = ds.batch(list(range(B)))
    runs = {"forwards": lambda: ensemble_members(model, xb, tfb, ei, K, seed=0),
            "evaluate_ensemble": lambda: evaluate_ensemble(model, ds, ei, B, members=K, seed=0, scaler=SCALER, baselines=()),
            "evaluate_ensemble fields": lambda: evaluate_ensemble(model, ds, ei, B, members=K, seed=0, scaler=SCALER, baselines=(),
                                                                  fields=spec)}
    times = {k: [] for k in runs}
    for p in range(1 + a.passes):
        for k, fn in runs.items():
            s = wall(fn)
            if p:
                times[k].append(s)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    f, e0, e1 = med["forwards"], med["evaluate_ensemble"], med["evaluate_ensemble fields"]
    say(f"evaluate_ensemble, {2 * B} windows in 2 batches, K = {K}, L_in = {L_IN}, fp32: {e0 * 1e3:.1f} ms without fields, "
        f"{e1 * 1e3:.1f} ms with: +{(e1 - e0) / 2 * 1e3:.2f} ms per batch; the {K} no-grad forwards of one batch {f * 1e3:.1f} ms: "
        f"field scores / forwards = {(e1 - e0) / 2 / f:.4f}"
        + (" -- the scores cost MORE than the forwards they score" if (e1 - e0) / 2 > f else "")
        + f"; median of {a.passes} alternating passes")
    say(f"all passes, seconds: {times}")
    with open(a.out + ".json", "w") as fh:
        json.dump(dict(device=dev_name, plan=dict(tile=T, lds_bytes=lds, workspace_bytes=ws), pair_terms=terms, kernel=kern,
                       update_wall_s=u, torch_wall_s=tt, torch_rel_diff=dict(energy=rel_es, variogram=rel_vs),
                       wall=dict(B=B, L_in=L_IN, median_s=med, all_s=times)), fh, indent=1)
    with open(a.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
