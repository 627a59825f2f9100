"""Per-case table of the hard-input suite (tests/hard_inputs.py): need_cpu (plain fp32 PyTorch on the CPU against float64),
need_gpu (the HIP kernel against float64), their ratio and the bar in force, for every tensor of every case of
tests/test_gpu_hard_inputs.py that has a CPU comparator, followed by the K and FLOOR the rule of the suite derives from
the table.  Measuring needs a GPU; --save keeps the measurements, and --load prints the table from them again (the bar and
verdict columns follow the K and FLOOR in force).  Its output is profiles/hard_inputs.txt:

    python tools/hard_inputs_report.py --save measured.json > profiles/hard_inputs.txt
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tec-mollm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from tests import hard_inputs as HI  # noqa: E402


BEFORE = os.path.join(ROOT, "profiles", "hard_inputs_spatial_before.txt")     # need_gpu measured before a kernel change


def collect(dev):
    from tecmollm import ops, rng
    rows, extras = [], {}
    for shape, *_ in HI.LN_SHAPES:
        e, x, _ = HI.ln_run(ops, rng, dev, shape, HI.LN_BWD if shape == "mixed768" else ("plain",))
        rows += HI.measure(e)
        extras.update({f"ln/{shape}/{k}": v for k, v in x.items()})
    for name in HI.GN_SHAPES:
        e, x, _ = HI.gn_run(ops, dev, name)
        rows += HI.measure(e)
        extras.update({f"gn/{name}/{k}": v for k, v in x.items()})
    for T in HI.ATT_SHORT + HI.ATT_LONG:
        for inst in HI.ATT_INST:
            for fam in HI.SOFTMAX_FAMILIES:
                e, x = HI.att_run(ops, rng, dev, fam, T, inst)
                rows += HI.measure(e)
                extras.update({f"att/{fam}/T{T}/{inst}/{k}": v for k, v in x.items() if v is not True})
    e, x = HI.conv_stats_run(ops, rng, dev)
    rows += HI.measure(e)
    extras.update(x)
    from oracle import ref_cpu as R
    for v2 in (True, False):
        os.environ.pop("TECM_SPATIAL_BWD2", None)
        os.environ["TECM_SPATIAL_V2"] = "1" if v2 else "0"
        for graph in HI.SPATIAL_GRAPHS:
            for variation in HI.SPATIAL_VARIATIONS:
                e, x = HI.spatial_run(R, dev, graph, variation, "fwd2_bwd2/" if v2 else "fwd_bwd/")
                rows += HI.measure(e)
    os.environ.pop("TECM_SPATIAL_V2", None)
    return rows, extras


def derive(rows):
    """(K, FLOOR, largest ratio, largest need_gpu among CPU-exact cases) by the rule in tests/hard_inputs.py."""
    ratio = max((ng / nc for _, nc, ng in rows if ng <= HI.BAR and nc >= HI.EXACT), default=0.0)
    k = 2.0 ** math.ceil(math.log2(max(2 * ratio, 1.0)))
    exact = max((ng for _, nc, ng in rows if nc < HI.EXACT and ng <= HI.BAR), default=0.0)
    return k, float(f"{2 * exact:.3g}"), ratio, exact


def render(device, rows, extras):
    k, floor, ratio, exact = derive(rows)
    print(f"# hard-input suite on {device}: need = smallest t with |got - ref| <= t (|ref| + 0.1 rms_row + 0.01 rms_all)")
    print(f"# BAR {HI.BAR:g}; in force: K {HI.K:g}, FLOOR {HI.FLOOR:g}")
    print(f"# derived from this table: largest need_gpu / need_cpu over cases under BAR with need_cpu >= {HI.EXACT:g}: {ratio:.3g} "
          f"-> K {k:g}; largest need_gpu with need_cpu < {HI.EXACT:g}: {exact:.3g} -> FLOOR {floor:g}")
    print(f"{'case':58s} {'need_cpu':>10s} {'need_gpu':>10s} {'ratio':>8s} {'bar':>9s}  verdict")
    for lab, nc, ng in rows:
        r = ng / nc if nc > 0 else float("inf") if ng > 0 else 0.0
        print(f"{lab:58s} {nc:10.3g} {ng:10.3g} {r:8.3g} {HI.bar_in_force(nc):9.3g}  {'ok' if HI.passes(ng, nc) else 'MISS'}")
    if os.path.exists(BEFORE):
        print("# kernel change: spatial_bwd / spatial_bwd2 take the self loop's dalpha off every dalpha of a target "
              "(need_gpu before, from profiles/hard_inputs_spatial_before.txt -> after, this table)")
        now = {lab: ng for lab, _, ng in rows}
        for line in open(BEFORE):
            if not line.startswith("#") and line.split():
                lab, old = line.split()
                print(f"{lab:58s} {float(old):10.3g} -> {now[lab]:10.3g}")
    print("# other checks (ratios: <= 1 passes)")
    for kx, v in extras.items():
        print(f"{kx:58s} {v if isinstance(v, bool) else format(v, '.3g')}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--save", metavar="JSON", help="also write the measurements (device, rows, other checks) to this file")
    ap.add_argument("--load", metavar="JSON", help="print the table from saved measurements, with the K and FLOOR now in force; needs no GPU")
    args = ap.parse_args()
    if args.load:
        with open(args.load) as f:
            m = json.load(f)
        device, rows, extras = m["device"], [tuple(r) for r in m["rows"]], m["extras"]
    else:
        rows, extras = collect(torch.device("cuda"))
        device = torch.cuda.get_device_name(0)
    if args.save:
        os.makedirs(os.path.dirname(os.path.abspath(args.save)), exist_ok=True)
        with open(args.save, "w") as f:
            json.dump({"device": device, "rows": rows, "extras": extras}, f)
    render(device, rows, extras)


if __name__ == "__main__":
    main()
