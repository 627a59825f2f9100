"""Host-side checks of the forecast combination (no GPU): the numpy restatement against `lstsq` and hand-worked cases, the
drop rule, the fallbacks, the 12-node world's held-out numbers, the launchers' refusals, the C ABI and the build lists, the
files and the name rules."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from tests import combine_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


members_and_truth = CR.members_and_truth


# ------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("M", [1, 2, 3, 5, 8])
def test_restatement_equals_lstsq_with_a_column_of_ones(M):
    preds, y = members_and_truth(M, 200, 2, 3, M)
    weight, intercept, status, dropped, cond = CR.solve(CR.moments(preds, y))
    assert weight.shape == (1, 2, M, 3) and not status.any() and not dropped.any() and cond.max() <= 1e4
    for h in range(2):
        for i in range(3):
            X = np.stack([np.ones(200)] + [p[:, h, i].astype(np.float64) for p in preds], axis=1)
            want = np.linalg.lstsq(X, y[:, h, i].astype(np.float64), rcond=None)[0]
            assert abs(intercept[0, h, i] - want[0]) <= 1e-9 and np.abs(weight[0, h, :, i] - want[1:]).max() <= 1e-9


def test_one_member_by_hand_and_the_moment_layout():
    """p = (0, 1, 2, 3), t = (1, 3, 5, 7) = 1 + 2 p: n = 4, sum p = 6, sum t = 16, sum pp = 14, sum pt = 34, sum tt = 84;
    C = 14 - 4 * 1.5^2 = 5, c = 34 - 4 * 1.5 * 4 = 10, w = 2, a = 4 - 2 * 1.5 = 1.  The fifth sample is skipped."""
    p = np.array([0, 1, 2, 3, np.nan], dtype=np.float32).reshape(5, 1, 1)
    t = np.array([1, 3, 5, 7, 9], dtype=np.float32).reshape(5, 1, 1)
    st = CR.moments([p], t)
    assert CR.moment_count(1) == 7 and st.shape == (1, 1, 7, 1)
    assert st[0, 0, :, 0].tolist() == [4.0, 6.0, 16.0, 14.0, 34.0, 84.0, 1.0]
    assert [CR.moment_index(1, a, b) for a in range(3) for b in range(a, 3)] == [0, 1, 2, 3, 4, 5]
    assert CR.moment_count(8) == 56 and CR.moment_index(8, 9, 9) == 54
    weight, intercept, status, dropped, _ = CR.solve(st)
    assert weight[0, 0, 0, 0] == 2.0 and intercept[0, 0, 0] == 1.0 and status[0, 0, 0] == 0 and dropped[0, 0, 0] == 0
    blend = CR.apply(weight, intercept, [p])
    assert blend[:4, 0, 0].tolist() == [1.0, 3.0, 5.0, 7.0] and np.isnan(blend[4, 0, 0])
    # ridge pulls the weight from 2 towards the prior 1: (10 + r*4*1) / (5 + r*4)
    weight, _, _, _, _ = CR.solve(st, ridge=0.5)
    assert abs(weight[0, 0, 0, 0] - 12.0 / 7.0) <= 1e-15


def test_groups_skip_bad_ids_and_leave_absent_groups_alone():
    preds, y = members_and_truth(3, 9, 2, 4, 2)
    ids = np.array([0, 2, 0, 5, 2, -1, 0, 2, 2])
    base = np.full((3, 2, CR.moment_count(2), 4), 7.5)
    st = CR.moments(preds, y, ids, 3, stats=base)
    assert (st[1] == 7.5).all() and st[0, 0, 0, 0] == 7.5 + 3 and st[2, 1, 0, 3] == 7.5 + 4
    keep = ids == 2
    assert np.array_equal(st[2] - 7.5, CR.moments([p[keep] for p in preds], y[keep])[0] + 7.5 - 7.5)


def test_an_exact_duplicate_is_dropped_and_changes_nothing():
    preds, y = members_and_truth(11, 120, 1, 5, 3)
    twin = [preds[0], preds[1], preds[0].copy(), preds[2]]
    weight, intercept, status, dropped, _ = CR.solve(CR.moments(twin, y))
    plain_w, plain_i, plain_s, _, _ = CR.solve(CR.moments(preds, y))
    assert (dropped == 0b100).all() and (status == CR.DROPPED).all() and not plain_s.any()
    assert (weight[:, :, 2] == 0).all()
    assert np.abs(weight[:, :, [0, 1, 3]] - plain_w).max() <= 1e-12 and np.abs(intercept - plain_i).max() <= 1e-12
    # a constant member has no variance: dropped by A_mm <= 0 or by its vanishing pivot
    const = [preds[0], np.full_like(preds[1], 3.25)]
    weight, _, _, dropped, _ = CR.solve(CR.moments(const, y))
    assert (dropped == 0b10).all() and (weight[:, :, 1] == 0).all()


def test_with_a_ridge_term_twins_share_the_weight():
    preds, y = members_and_truth(13, 120, 1, 5, 2)
    twin = [preds[0], preds[1], preds[0].copy()]
    weight, intercept, status, dropped, _ = CR.solve(CR.moments(twin, y), ridge=0.01)
    assert not status.any() and not dropped.any()
    assert np.abs(weight[:, :, 0] - weight[:, :, 2]).max() <= 1e-9
    pair_w, _, _, _, _ = CR.solve(CR.moments(preds, y), ridge=0.0)
    assert np.abs(weight[:, :, 0] + weight[:, :, 2] - pair_w[:, :, 0]).max() <= 0.05      # the pair carries the single's weight


def test_fallbacks_empty_few_and_nonfinite():
    preds, y = members_and_truth(17, 6, 1, 4, 2)
    ids = np.array([0, 0, 0, 0, 0, 1])                                     # group 1: one sample (FEW); group 2: none (EMPTY)
    st = CR.moments(preds, y, ids, 3)
    st[0, 0, 3, 2] = np.inf                                                # one moment of cell (0, 0, 2)
    w0 = np.array([0.25, 0.75])
    weight, intercept, status, dropped, _ = CR.solve(st, 0.0, w0)
    assert status[2].tolist() == [[CR.EMPTY] * 4] and status[1].tolist() == [[CR.FEW] * 4]
    assert status[0, 0].tolist() == [0, 0, CR.NONFINITE, 0] and not dropped.any()
    for g, i in ((2, 0), (1, 1), (0, 2)):
        assert weight[g, 0, :, i].tolist() == [0.25, 0.75]
    assert (intercept[2] == 0).all() and intercept[0, 0, 2] == 0
    p5 = [float(p[5, 0, 1]) for p in preds]
    assert intercept[1, 0, 1] == float(y[5, 0, 1]) - (0.25 * p5[0] + 0.75 * p5[1])
    # four samples for two members is exactly M + 2: solved
    st4 = CR.moments([p[:4] for p in preds], y[:4])
    assert not CR.solve(st4)[2].any() and (CR.solve(CR.moments([p[:3] for p in preds], y[:3]))[2] == CR.FEW).all()


def test_the_world_in_sample_property_and_held_out_numbers():
    """The 12-node seasonal AR(1): members ("mean", "last", "periodic"), per-cell weights, scaled domain."""
    y = CR.world_series()
    r0, r1 = CR.held_out(y, ridge=0.0), CR.held_out(y, ridge=0.01)
    got = {"c0": r0["combination"], "c1": r1["combination"], "mean": r0["mean"], "periodic": r0["periodic"], "last": r0["last"]}
    want = {"c0": 1.118, "c1": 1.108, "mean": 1.208, "periodic": 1.363, "last": 1.627}
    for k in want:
        assert abs(got[k] - want[k]) <= 5e-4, (k, got[k])
    assert all(r0["combination"] < r0[k] for k in ("mean", "last", "periodic"))
    d = r0["dropped"][0]
    assert (d[11] == 0b100).all() and not d[:11].any() and not r1["dropped"].any()
    # least squares is never beaten in-sample by a single member, per cell, up to the blend's one float32 rounding
    blend, truth = r0["blend_fit"].astype(np.float64), r0["truth_fit"].astype(np.float64)
    res = truth - blend
    slack = 2.0 ** -23 * (np.abs(res) * np.abs(blend)).sum(axis=0)
    for k, p in r0["members_fit"].items():
        assert ((res ** 2).sum(axis=0) <= ((truth - p.astype(np.float64)) ** 2).sum(axis=0) + slack).all(), k


# ------------------------------------------------------------------------------------ the launchers' refusals
def _buf():
    buf = (ctypes.c_double * 8)()                                          # a real, aligned host address: never dereferenced
    return buf, ctypes.addressof(buf)


def _operands(d, a, M):
    for m in range(M):
        d.member[m].base, d.member[m].stride_s, d.member[m].stride_h, d.member[m].stride_i = a, 1, 1, 1


def _moments_descriptor(members=2, **over):
    from tecmollm import _lib
    buf, a = _buf()
    f = dict(S=1, H=1, G=1, I=1, M=members, stats=a, group=None, err_flag=a)
    target = over.pop("target", a)
    f.update(over)
    d = _lib.TecmCombineMoments(**f)
    _operands(d, a, max(0, min(members, 8)))
    d.target.base = target
    d._keep = buf
    return d


def _solve_descriptor(**over):
    from tecmollm import _lib
    buf, a = _buf()
    f = dict(stats=a, s_stride_g=1, s_stride_h=1, s_stride_k=1, s_stride_i=1, G=1, H=1, I=1, M=2, ridge=0.0, weight=a,
             intercept=a, status=a, dropped=a)
    w0 = over.pop("w0", None)
    f.update(over)
    d = _lib.TecmCombineSolve(**f)
    if w0 is not None:
        d.w0[1] = w0
    d._keep = buf
    return d


def _apply_descriptor(members=2, **over):
    from tecmollm import _lib
    buf, a = _buf()
    f = dict(S=1, H=1, G=1, I=1, M=members, weight=a, intercept=a, out=a, group=None, err_flag=a)
    null_member = over.pop("null_member", False)
    f.update(over)
    d = _lib.TecmCombineApply(**f)
    _operands(d, a, max(0, min(members, 8)))
    if null_member:
        d.member[1].base = None
    d._keep = buf
    return d


def _null_member_moments():
    d = _moments_descriptor()
    d.member[0].base = None
    return d


@pytest.mark.parametrize("make, fn, over, text", [
    (_moments_descriptor, "tecm_combine_moments", dict(members=0), b"M must be in [1, 8]"),
    (_moments_descriptor, "tecm_combine_moments", dict(members=9), b"M must be in [1, 8]"),
    (_moments_descriptor, "tecm_combine_moments", dict(target=None), b"null pointer"),
    (_moments_descriptor, "tecm_combine_moments", dict(stats=None), b"null pointer"),
    (_moments_descriptor, "tecm_combine_moments", dict(err_flag=None), b"null pointer"),
    (_moments_descriptor, "tecm_combine_moments", dict(S=0), b"bad shape"),
    (_moments_descriptor, "tecm_combine_moments", dict(G=65536), b"<= 65535"),
    (_moments_descriptor, "tecm_combine_moments", dict(H=4 * 65535 + 1), b"<= 65535"),
    (_moments_descriptor, "tecm_combine_moments", dict(I=64 << 24), b"2^24 blocks"),
    (_solve_descriptor, "tecm_combine_solve", dict(M=0), b"M must be in [1, 8]"),
    (_solve_descriptor, "tecm_combine_solve", dict(M=9), b"M must be in [1, 8]"),
    (_solve_descriptor, "tecm_combine_solve", dict(weight=None), b"null pointer"),
    (_solve_descriptor, "tecm_combine_solve", dict(dropped=None), b"null pointer"),
    (_solve_descriptor, "tecm_combine_solve", dict(I=0), b"bad shape"),
    (_solve_descriptor, "tecm_combine_solve", dict(ridge=-1e-3), b"ridge must be finite and >= 0"),
    (_solve_descriptor, "tecm_combine_solve", dict(ridge=float("nan")), b"ridge must be finite and >= 0"),
    (_solve_descriptor, "tecm_combine_solve", dict(w0=float("inf")), b"prior must be finite"),
    (_solve_descriptor, "tecm_combine_solve", dict(G=65535, H=65535, I=1 << 20), b"blocks of 256 cells"),
    (_apply_descriptor, "tecm_combine_apply", dict(members=0), b"M must be in [1, 8]"),
    (_apply_descriptor, "tecm_combine_apply", dict(members=9), b"M must be in [1, 8]"),
    (_apply_descriptor, "tecm_combine_apply", dict(null_member=True), b"null pointer (member 1)"),
    (_apply_descriptor, "tecm_combine_apply", dict(out=None), b"null pointer"),
    (_apply_descriptor, "tecm_combine_apply", dict(intercept=None), b"null pointer"),
    (_apply_descriptor, "tecm_combine_apply", dict(H=0), b"bad shape"),
    (_apply_descriptor, "tecm_combine_apply", dict(H=4 * 65535 + 1), b"<= 65535"),
])
def test_the_launchers_reject_bad_descriptors_before_any_device_call(make, fn, over, text):
    from tecmollm import _lib
    d = make(**over)
    rc = getattr(_lib.lib(), fn)(ctypes.byref(d), None)
    assert rc == -1, (over, rc)                                            # TECM_E_ARG
    assert text in _lib.lib().tecm_last_error(), (over, _lib.lib().tecm_last_error())


def test_the_launchers_reject_a_null_descriptor_a_null_member_and_misaligned_pointers():
    from tecmollm import _lib
    assert _lib.lib().tecm_combine_moments(ctypes.byref(_null_member_moments()), None) == -1
    assert b"null pointer (member 0)" in _lib.lib().tecm_last_error()
    for fn, make, field in (("tecm_combine_moments", _moments_descriptor, "stats"), ("tecm_combine_solve", _solve_descriptor, "weight"),
                            ("tecm_combine_apply", _apply_descriptor, "intercept")):
        assert getattr(_lib.lib(), fn)(None, None) == -1 and b"null descriptor" in _lib.lib().tecm_last_error()
        d = make()
        setattr(d, field, getattr(d, field) + 2)
        assert getattr(_lib.lib(), fn)(ctypes.byref(d), None) == -2, fn    # TECM_E_ALIGN
        assert b"aligned" in _lib.lib().tecm_last_error()


def test_the_wrappers_refuse_host_tensors_and_bad_arguments():
    import torch
    from tecmollm import combine as CB
    from tecmollm._lib import TecmError
    cm = CB.CombinationMoments(["a", "b"], 2, 3, device="cpu")
    assert cm.stats.shape == (1, 2, CR.moment_count(2), 3) and cm.K == 11
    t = torch.zeros(4, 2, 3)
    with pytest.raises(TecmError, match="must live on the GPU"):
        cm.update([t, t], t)
    with pytest.raises(ValueError, match="2 members"):
        cm.update([t], t)
    for kw, text in ((dict(ridge=-1.0), "ridge"), (dict(ridge=float("nan")), "ridge"), (dict(prior=[1.0]), "prior"),
                     (dict(prior=[1.0, float("inf")]), "prior"), (dict(pool="node"), "pool")):
        with pytest.raises(ValueError, match=text):
            cm.fit(**kw)
    for bad in ([], [f"m{i}" for i in range(9)]):
        with pytest.raises(ValueError, match="1 to 8 members"):
            CB.CombinationMoments(bad, 2, 3, device="cpu")
    with pytest.raises(ValueError, match="unique"):
        CB.CombinationMoments(["a", "a"], 2, 3, device="cpu")
    with pytest.raises(ValueError, match="at least one"):
        CB.CombinationMoments(["a"], 0, 3, device="cpu")
    assert cm.pooled_stats("horizon").shape == (1, 2, 11, 1) and cm.pooled_stats("all").shape == (1, 1, 11, 1)


# ------------------------------------------------------------------------------------ the C ABI and the build
def test_abi_struct_sizes_exports_and_the_build_lists():
    import tecmollm
    import __graft_entry__ as G
    from tecmollm import _lib
    from tecmollm import combine as CB
    header = open(os.path.join(ROOT, "include", "tecmollm.h"), encoding="utf-8").read()
    assert _lib.ABI_VERSION == 21 and "#define TECM_ABI_VERSION 21" in header
    for name, value in (("TECM_COMBINE_MAX_MEMBERS", 8), ("TECM_COMBINE_EMPTY", 1), ("TECM_COMBINE_FEW", 2),
                        ("TECM_COMBINE_DROPPED", 4), ("TECM_COMBINE_NONFINITE", 8)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1)) == value == getattr(_lib, name)
    assert float(re.search(r"#define\s+TECM_COMBINE_PIVOT_TOL\s+(\S+)", header).group(1)) == _lib.TECM_COMBINE_PIVOT_TOL == CR.PIVOT_TOL
    assert (CB.EMPTY, CB.FEW, CB.DROPPED, CB.NONFINITE, CB.MAX_MEMBERS) == (CR.EMPTY, CR.FEW, CR.DROPPED, CR.NONFINITE, CR.MAX_MEMBERS)
    assert ctypes.sizeof(_lib.TecmCombineOperand) == 32
    assert ctypes.sizeof(_lib.TecmCombineMoments) == 32 * 9 + 8 + 4 + 4 + 8 + 4 + 4 + 8 * 3
    assert ctypes.sizeof(_lib.TecmCombineSolve) == 8 * 5 + 4 + 4 + 8 + 4 + 4 + 8 + 8 * 8 + 8 * 4
    assert ctypes.sizeof(_lib.TecmCombineApply) == 32 * 8 + 8 + 4 + 4 + 8 + 4 + 4 + 8 * 5 + 8 * 4 + 8 * 4 + 8 * 2
    assert _lib.TecmCombineMoments.target.offset == 256 and _lib.TecmCombineSolve.w0.offset == 72
    # field for field: the names of every struct in the header, in order
    for name in ("TecmCombineOperand", "TecmCombineMoments", "TecmCombineSolve", "TecmCombineApply"):
        body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", header).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.sub(r"\[.*\]", "", decl.split()[-1]).lstrip("*") for part in body.split(";") for decl in part.split(",")
                  if decl.strip()]
        assert fields == [f[0] for f in getattr(_lib, name)._fields_], name
    for name in ("tecm_combine_moments", "tecm_combine_solve", "tecm_combine_apply"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name) and f"int {name}(" in header
    assert "combine.hip" in G.SOURCES
    rules = G.SPILL_CEILINGS["combine.hip"]
    frags = {f for f, _, _ in rules}
    assert frags == {f"combine_{k}_kernelILi{mb}E" for k in ("moments", "solve") for mb in (1, 2, 4, 8)} | {"combine_apply_kernel"}
    assert all(field == "ScratchSize [bytes/lane]" and ceiling == 0 for _, field, ceiling in rules)
    for name in ("Combination", "CombinationMoments", "fit_combination", "write_combination"):
        assert name in tecmollm.__all__ and callable(getattr(tecmollm, name))
    assert CB.moment_count(4) == CR.moment_count(4) == 22 and CB.moment_index(4, 2, 5) == CR.moment_index(4, 2, 5)


# ------------------------------------------------------------------------------------ files and names
def _fitted(pool="cell", members=("mean", "last", "periodic"), name="Combination", G=1):
    from tecmollm import combine as CB
    H, N, M = 3, 6, len(members)
    Hs, Ns = (H, N) if pool == "cell" else ((H, 1) if pool == "horizon" else (1, 1))
    rng = np.random.default_rng(5)
    status = np.zeros((G, Hs, Ns), dtype=np.int32)
    dropped = np.zeros((G, Hs, Ns), dtype=np.uint8)
    status[0, 0, 0], dropped[0, 0, 0] = CB.DROPPED, 0b10
    status[-1, -1, -1] = CB.FEW
    names = [CB.member_name(m) for m in members]
    return CB.Combination(rng.standard_normal((G, Hs, M, Ns)), rng.standard_normal((G, Hs, Ns)), status, dropped,
                          np.full((G, Hs, Ns), 40.0), np.zeros((G, Hs, Ns)), names, (H, N), 0.01, pool, name, list(members))


@pytest.mark.parametrize("pool", ["cell", "horizon", "all"])
def test_save_load_and_write_combination(tmp_path, pool):
    import csv
    from tecmollm import combine as CB
    comb = _fitted(pool, G=2)
    assert comb.weight.shape == (2, 3, 3, 6) and comb.intercept.shape == comb.status.shape == comb.counts.shape == (2, 3, 6)
    if pool != "cell":
        assert comb.weight.strides[3] == 0 and comb.intercept.strides[2] == 0      # stride-0 views over the pooled axes
    if pool == "all":
        assert comb.weight.strides[1] == 0
    path = comb.save(str(tmp_path / "comb.npz"))
    with np.load(path, allow_pickle=False) as z:                            # arrays and strings only
        assert all(z[k].dtype.kind in "fiuU" for k in z.files)
    back = CB.Combination.load(path)
    for k in ("weight", "intercept", "status", "dropped", "counts", "skipped"):
        assert np.array_equal(getattr(back, k), getattr(comb, k)) and getattr(back, k).dtype == getattr(comb, k).dtype, k
    assert (back.member_names, back.ridge, back.pool, back.name, back.G, back.H, back.N) == (["mean", "last", "periodic"], 0.01, pool,
                                                                                       "Combination", 2, 3, 6)
    assert back.members == ["mean", "last", "periodic"]
    paths = CB.write_combination(comb, str(tmp_path), grid=(2, 3))
    with np.load(paths["npz"]) as z:
        assert z["weight"].shape == (2, 3, 3, 2, 3) and z["intercept"].shape == z["status"].shape == (2, 3, 2, 3)
        assert np.array_equal(z["weight"].reshape(2, 3, 3, 6), comb.weight) and z["member_names"].tolist() == comb.member_names
    rows = list(csv.reader(open(paths["csv"], encoding="utf-8")))
    assert rows[0] == ["group", "horizon", "weight_mean", "weight_last", "weight_periodic", "intercept", "cells_dropped", "cells_fallback"]
    assert len(rows) == 1 + 2 * 3
    cells = {"cell": 1, "horizon": 6, "all": 6}[pool]
    assert rows[1][:2] == ["0", "0"] and int(rows[1][6]) == cells and float(rows[1][2]) == float(comb.weight[0, 0, 0].mean())
    assert int(rows[-1][7]) == cells
    with pytest.raises(ValueError, match="grid"):
        CB.write_combination(comb, str(tmp_path), grid=(2, 4))


def test_name_rules():
    from src.models.baselines import LinearBaseline
    from tecmollm import combine as CB
    from tecmollm import evaluate as E
    assert CB.check_members(("model", "mean", "last", "periodic")) == ["model", "mean", "last", "periodic"]
    for bad, text in ((("mean", "mean"), "unique"), ((), "1 to 8 members"), (("model",) * 9, "1 to 8 members"),
                      (("median",), "a member is"), ((3,), "a member is"), ((LinearBaseline(device="cpu"),), "must be fitted"),
                      ((_fitted(),), "cannot be a member")):
        with pytest.raises(ValueError, match=text):
            CB.check_members(bad)
    comb = _fitted(name="Blend")
    assert E.baseline_name(comb) == "Blend"
    assert E.baseline_names(("mean", comb, "last")) == ["HistoricalAverage", "Blend", "Persistence"]
    for name, others in (("HistoricalAverage", ("mean",)), ("Blend", (comb,))):
        with pytest.raises(ValueError, match="collides"):
            E.baseline_names(others + (_fitted(name=name),))
    with pytest.raises(ValueError, match="name other than"):
        _fitted(name=E.MODEL_NAME)
    # a combination fitted with groups needs the evaluation's groups to match
    grouped = _fitted(G=3)
    with pytest.raises(ValueError, match="fitted with 3 groups"):
        E.baseline_names((grouped,))
    with pytest.raises(ValueError, match="fitted with 3 groups"):
        E.baseline_names((grouped,), groups=object(), num_groups=2)
    assert E.baseline_names((grouped,), groups=object(), num_groups=3) == ["Combination"]
    # members that are objects come back by name
    with pytest.raises(ValueError, match="do not match"):
        CB.Combination(comb.weight, comb.intercept, comb.status, comb.dropped, comb.counts, comb.skipped, comb.member_names,
                       (3, 6), members=["mean", "last"])
    lone = CB.Combination(comb.weight[:, :, :1], comb.intercept, comb.status, comb.dropped, comb.counts, comb.skipped, ["Linear"], (3, 6))
    assert lone.members == [None]
    with pytest.raises(ValueError, match="pass it again"):
        lone._member_forecasts(None, [0], None)
    with pytest.raises(ValueError, match="needs a forecast of every member"):
        comb.combine({"mean": None})
