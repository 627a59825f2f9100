"""Cost of the member reordering (reorder_members / tecm_member_reorder) at the workload shape: N = 2911, K = 16 members,
B = 16, L_out = 12, for both template sources -- a (K, B, L_out, N) member tensor (ECC) and K dated rows per window of a
(T, N) archive, time-major and node-major (the Schaake shuffle).  Recorded, not gated.

  * kernel time: a run of its own under `rocprofv3 --kernel-trace --stats` (a child process started before this one touches
    the GPU), read from the trace database, first launch of every variant dropped.  The launches walk a ring of RING buffer
    sets (values, template, out: 107 MB each), 430 MB in all, so that no launch finds its operands in the 256 MiB Infinity
    Cache; the archive of the dated variants (26 MB) is read again by every launch, as it is in use;
  * call time: device events around CALLS calls of `reorder_members` on the same ring (launch overhead included);
  * the torch route on the device: the template materialised (for the dated variants by an index gather), two stable
    argsorts of it, a stable sort of the values, take_along_dim; device events, the same ring; and whether its result has
    the kernel's bits;
  * the floor: the bytes the algorithm needs (2 K floats in, K floats out per cell) over the HBM rate a streaming kernel
    achieves (6.3 TB/s of the 8 TB/s peak).

    python tools/coherence_bench.py [--out PREFIX] [--no-profile]        # writes PREFIX.json and PREFIX.txt
"""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tec-mollm_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

N, K, B, L_OUT, T_ARCHIVE = 2911, 16, 16, 12, 2208
RING, PROFILE_LAUNCHES, CALLS, TORCH_CALLS = 4, 8, 40, 8
HBM_ACHIEVABLE = 6.3e12
VARIANTS = ("member tensor", "dated rows, (T, N) archive", "dated rows, (N, T) archive")
ALGO_BYTES = 3 * K * B * L_OUT * N * 4


def operands():
    """[(values, template, rows or None, out)] * RING per variant, seeded."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    shape = (K, B, L_OUT, N)
    ring = [(torch.randn(shape, device="cuda", generator=g), torch.randn(shape, device="cuda", generator=g),
             torch.empty(shape, device="cuda")) for _ in range(RING)]
    archive = torch.randn(T_ARCHIVE, N, device="cuda", generator=g)
    node_major = archive.t().contiguous().t()                               # (T, N) view of (N, T) storage
    rows = [torch.randint(0, T_ARCHIVE - L_OUT + 1, (B, K), device="cuda", generator=g, dtype=torch.int32) for _ in range(RING)]
    return {VARIANTS[0]: [(v, t, None, o) for v, t, o in ring],
            VARIANTS[1]: [(v, archive, r, o) for (v, _, o), r in zip(ring, rows)],
            VARIANTS[2]: [(v, node_major, r, o) for (v, _, o), r in zip(ring, rows)]}


def kernels_only():
    """The child run under the profiler: per variant one warm-up launch and PROFILE_LAUNCHES more, round the ring."""
    import torch
    from tecmollm import reorder_members
    ops = operands()
    for name in VARIANTS:
        for n in range(1 + PROFILE_LAUNCHES):
            v, t, r, o = ops[name][n % RING]
            reorder_members(v, t, rows=r, out=o)
    torch.cuda.synchronize()


def profile_kernels(timeout=420):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "coherence", "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=td)
        dbs = glob.glob(os.path.join(td, "**", "*_results.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-1500:]}")
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, start, end from kernels order by start").fetchall()
    us = [(e - s) / 1e3 for name, s, e in rows if "member_reorder_kernel" in name]
    per = 1 + PROFILE_LAUNCHES
    if len(us) != per * len(VARIANTS):
        raise RuntimeError(f"expected {per * len(VARIANTS)} launches of member_reorder_kernel, saw {len(us)}")
    out = {}
    for n, name in enumerate(VARIANTS):
        u = us[n * per + 1:(n + 1) * per]
        out[name] = dict(launches=len(u), us=float(np.median(u)), us_min=float(np.min(u)), us_max=float(np.max(u)))
    return out


def event_us(fn, sets, calls):
    """Microseconds per call of fn(*set) round the ring, device events around `calls` calls, after one call per set."""
    import torch
    for s in sets:
        fn(*s)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for n in range(calls):
        fn(*sets[n % len(sets)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def torch_route(v, t, r, o):
    """The same reordering with torch ops on a materialised template."""
    import torch
    if r is not None:
        idx = r.t().to(torch.int64).unsqueeze(-1) + torch.arange(L_OUT, device=v.device)       # (K, B, H) rows of the archive
        t = t[idx]                                                                               # (K, B, H, N)
    rank = torch.argsort(torch.argsort(t, dim=0, stable=True), dim=0, stable=True)
    o.copy_(torch.take_along_dim(torch.sort(v, dim=0, stable=True).values, rank, dim=0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coherence"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child run (kernel times: not measured)")
    ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    kern = {} if a.no_profile else profile_kernels()                       # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("coherence_bench.py measures on the GPU; none found")
    from tecmollm import reorder_members
    dev_name = torch.cuda.get_device_name(0)
    lines = [f"# {dev_name}; N = {N}, K = {K}, B = {B}, L_out = {L_OUT}, archive T = {T_ARCHIVE}; ring of {RING} buffer sets; "
             f"python tools/coherence_bench.py" + (" --no-profile" if a.no_profile else "")]

    def say(s):
        lines.append(s)
        print(s, flush=True)
    floor_us = ALGO_BYTES / HBM_ACHIEVABLE * 1e6
    say(f"algorithmic bytes per call: {ALGO_BYTES / 1e6:.1f} MB ({2 * ALGO_BYTES / 3e6:.1f} MB in, {ALGO_BYTES / 3e6:.1f} MB out); "
        f"at the achievable HBM rate of {HBM_ACHIEVABLE / 1e12:.1f} TB/s: {floor_us:.1f} us")
    ops = operands()
    rows = {}
    for name in VARIANTS:
        sets = ops[name]
        call = event_us(lambda v, t, r, o: reorder_members(v, t, rows=r, out=o), sets, CALLS)
        ours = sets[0][3].clone()
        tor = event_us(torch_route, sets, TORCH_CALLS)
        same = bool(torch.equal(ours.view(torch.int32), sets[0][3].view(torch.int32)))
        row = dict(call_us_events=call, torch_us_events=tor, torch_identical_bits=same)
        if name in kern:
            k = kern[name]
            row.update(kernel=k, kernel_bytes_per_s=ALGO_BYTES / (k["us"] * 1e-6), share_of_achievable_hbm=floor_us / k["us"])
            say(f"{name}: kernel {k['us']:.1f} us (min {k['us_min']:.1f}, max {k['us_max']:.1f}; rocprofv3 kernel trace, "
                f"{k['launches']} launches) = {ALGO_BYTES / k['us'] / 1e6:.2f} TB/s of algorithmic bytes, "
                f"{100 * floor_us / k['us']:.0f} % of the achievable HBM rate (the floor is the bytes)")
        else:
            say(f"{name}: kernel time: not measured")
        say(f"{name}: reorder_members call {call:.1f} us (device events, {CALLS} calls); torch route {tor:.0f} us "
            f"({TORCH_CALLS} calls) = {tor / call:.1f} x"
            + ("" if tor > call else " -- the kernel is NOT faster than the torch route")
            + f"; torch result has the kernel's bits: {same}")
        rows[name] = row
    with open(a.out + ".json", "w") as fh:
        json.dump(dict(device=dev_name, shape=dict(N=N, K=K, B=B, L_out=L_OUT, T_archive=T_ARCHIVE), ring=RING,
                       algorithmic_bytes=ALGO_BYTES, hbm_achievable_bytes_per_s=HBM_ACHIEVABLE, floor_us=floor_us,
                       variants=rows), fh, indent=1)
    with open(a.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
