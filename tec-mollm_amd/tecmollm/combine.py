"""Forecast combination on the device: a least-squares fit of the truth on several forecasts of it, with an intercept, per
cell (group of the window, horizon, node) -- Bates and Granger (1969), Granger and Ramanathan (1984).

The evaluation side scores every forecast alone; the first thing a forecaster does with several imperfect forecasts of the
same quantity is blend them.  `fit_combination` makes one `eval()` pass over a held-out split and feeds every batch's
member forecasts and targets, where they lie, to `tecm_combine_moments` (include/tecmollm.h (3l)): the (M+2) x (M+2) moment
matrix of [1, p_1 .. p_M, t] per cell is all a least-squares fit needs, it is additive over batches and ranks, and it is a
few MB where the forecasts of a split are hundreds.  `tecm_combine_solve` then solves every cell's small system in one
launch (a Cholesky factorisation that DROPS a member whose pivot vanishes: members that coincide in a cell, as "periodic"
and "last" do at horizon period - 1, leave the fit defined), and `Combination.combine` blends a batch (`tecm_combine_apply`).
With one member the fit is the per-cell affine recalibration a + w * model (MOS bias correction); with the window baselines
as members the intercept and the weights absorb the mismatch between the feature-scaled X they read and the target-scaled Y
they are scored against.  A fitted `Combination` is an element of `baselines=` everywhere a "Linear" is.

What this is NOT.  The weights are unconstrained: neither non-negative nor summing to one.  They are fixed, not
time-varying.  Quantile and ensemble members are not combined.  The centred matrix is formed from uncentred float64
moments, so a member whose mean is large against its spread loses digits accordingly (the scaled domain keeps that small).
Fitting and scoring on the same split is in-sample and flatters the result: fit on one split, score on another.
"""
from __future__ import annotations

import csv
import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import TecmCombineApply, TecmCombineMoments, TecmCombineSolve, check, lib, stream_ptr
from .devcheck import check_device_errors, error_word
from .evaluate import KINDS, MODEL_NAME, _score_pass, baseline_forecast, baseline_name, check_grid

MAX_MEMBERS = _lib.TECM_COMBINE_MAX_MEMBERS
EMPTY, FEW, DROPPED, NONFINITE = (_lib.TECM_COMBINE_EMPTY, _lib.TECM_COMBINE_FEW, _lib.TECM_COMBINE_DROPPED,
                                  _lib.TECM_COMBINE_NONFINITE)
POOLS = ("cell", "horizon", "all")
MODEL_MEMBER = "model"      # the member spec that stands for the model's own output
DEFAULT_NAME = "Combination"


def moment_count(members: int) -> int:
    """K of `stats (G, H, K, I)`: the upper triangle of the (M+2) x (M+2) moment matrix and `skipped`."""
    return (members + 2) * (members + 3) // 2 + 1


def moment_index(members: int, a: int, b: int) -> int:
    """The position of moment (a, b), a <= b, of z = [1, p_1 .. p_M, t] in the K statistics of a cell."""
    return a * (members + 2) - a * (a - 1) // 2 + (b - a)


def member_name(spec) -> str:
    """The name of one member: "model", a kind string of `window_baseline`, or the `baselines=` name of a fitted
    `SarimaBaseline` / `LinearBaseline` / `AnalogBaseline` ("SARIMA", "Linear", "Analog")."""
    if isinstance(spec, str):
        if spec == MODEL_MEMBER or spec in KINDS:
            return spec
        raise ValueError(f"a member is {MODEL_MEMBER!r}, one of {sorted(KINDS)} or a fitted baseline object, got {spec!r}")
    if isinstance(spec, Combination):
        raise ValueError("a Combination cannot be a member of a combination")
    try:
        return baseline_name(spec)
    except ValueError as e:
        raise ValueError(f"a member is {MODEL_MEMBER!r}, one of {sorted(KINDS)} or a fitted baseline object: {e}") from None


def check_members(members) -> list:
    """The member names of `members`; raises ValueError unless there are 1..8 of them with unique names."""
    specs = list(members)
    if not 1 <= len(specs) <= MAX_MEMBERS:
        raise ValueError(f"a combination takes 1 to {MAX_MEMBERS} members, got {len(specs)}")
    names = [member_name(s) for s in specs]
    if len(set(names)) != len(names):
        raise ValueError(f"member names must be unique, got {names}")
    return names


def _operand(t: torch.Tensor, name: str):
    from src.evaluation.metrics import _as_shi
    return _as_shi(t, name)


def _fill(slot, t: torch.Tensor, strides) -> None:
    slot.base, slot.stride_s, slot.stride_h, slot.stride_i = t.data_ptr(), strides[0], strides[1], strides[2]


def _group_ids(groups: Optional[torch.Tensor], S: int, G: int):
    if groups is None:
        if G > 1:
            raise ValueError(f"{G} groups need one group id per sample (groups=)")
        return None
    _lib.require_gpu_tensor(groups, "groups", torch.int32)
    if groups.shape != (S,):
        raise ValueError(f"groups must hold one id per sample: {tuple(groups.shape)} for {S} samples")
    return groups.contiguous()


class CombinationMoments:
    """The sufficient statistics of the per-cell fit, accumulated on the device: update(preds, y, groups) per batch (one
    launch of `tecm_combine_moments`; no atomics, so the same batches give the same bits), merge_() across ranks, fit()."""

    def __init__(self, members: Sequence[str], num_horizons: int, num_nodes: int, num_groups: int = 1, device="cuda"):
        self.member_names = [str(m) for m in members]
        if not 1 <= len(self.member_names) <= MAX_MEMBERS:
            raise ValueError(f"a combination takes 1 to {MAX_MEMBERS} members, got {len(self.member_names)}")
        if len(set(self.member_names)) != len(self.member_names):
            raise ValueError(f"member names must be unique, got {self.member_names}")
        self.M = len(self.member_names)
        self.H, self.I, self.G = int(num_horizons), int(num_nodes), int(num_groups)
        if min(self.H, self.I, self.G) < 1:
            raise ValueError("CombinationMoments needs at least one horizon, one node and one group")
        self.K = moment_count(self.M)
        # [g][h][k][i]: node-contiguous, the layout the kernel's lanes read and write
        self.stats = torch.zeros(self.G, self.H, self.K, self.I, device=device, dtype=torch.float64)

    def reset(self) -> None:
        self.stats.zero_()

    def update(self, preds, y: torch.Tensor, groups: Optional[torch.Tensor] = None) -> None:
        """`preds`: the M member forecasts, a sequence in member order or a dict by member name, each (S, H, N[, 1]) float32
        on the device with any strides; `y` the targets likewise; `groups` (S,) int32 on the device."""
        if isinstance(preds, dict):
            preds = [preds[n] for n in self.member_names]
        preds = list(preds)
        if len(preds) != self.M:
            raise ValueError(f"{self.M} members, got {len(preds)} forecasts")
        t, S, H, I, ts, th, ti = _operand(y, "y")
        if H != self.H or I != self.I:
            raise ValueError(f"shape mismatch: y {tuple(y.shape)}, horizons {self.H}, nodes {self.I}")
        d = TecmCombineMoments(S=S, H=H, G=self.G, I=I, M=self.M, stats=self.stats.data_ptr())
        keep = [t]
        for m, p in enumerate(preds):
            p, S2, H2, I2, ps, ph, pi = _operand(p, self.member_names[m])
            if (S2, H2, I2) != (S, H, I):
                raise ValueError(f"shape mismatch: member {self.member_names[m]} {tuple(p.shape)}, y {tuple(y.shape)}")
            keep.append(p)
            _fill(d.member[m], p, (ps, ph, pi))
        _fill(d.target, t, (ts, th, ti))
        ids = _group_ids(groups, S, self.G)
        errs = error_word(self.stats.device)
        d.group, d.err_flag = _lib.ptr(ids), errs.ptr()
        check(lib().tecm_combine_moments(C.byref(d), stream_ptr()), "tecm_combine_moments")
        if ids is not None:
            errs.post()                        # only a group id can set the word here

    def merge_(self, group=None) -> "CombinationMoments":
        """Sum the moments over the ranks of `group` with one all-reduce, in place: they are additive."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.stats, op=dist.ReduceOp.SUM, group=group)
        return self

    def pooled_stats(self, pool: str = "cell") -> torch.Tensor:
        """The moments the solve sees: as they are ("cell", (G, H, K, N)), summed over the nodes ("horizon", (G, H, K, 1)) or
        over nodes and horizons ("all", (G, 1, K, 1)), on the device."""
        if pool not in POOLS:
            raise ValueError(f"pool must be one of {POOLS}, got {pool!r}")
        if pool == "cell":
            return self.stats
        return self.stats.sum(dim=3, keepdim=True) if pool == "horizon" else self.stats.sum(dim=(1, 3), keepdim=True)

    def fit(self, ridge: float = 0.0, prior=None, pool: str = "cell", name: str = DEFAULT_NAME, members=None) -> "Combination":
        """Solve every cell (one launch of `tecm_combine_solve`).  `ridge` >= 0 shrinks the weights towards `prior` (default
        1 / M each; 1.0 for one member) by adding ridge * n to the diagonal; `pool` fits one system per cell, per (group,
        horizon) or per group, and the coefficients come back as stride-0 views over the pooled axes."""
        ridge = float(ridge)
        if not (ridge >= 0.0 and np.isfinite(ridge)):
            raise ValueError(f"ridge must be finite and >= 0, got {ridge}")
        w0 = np.full(self.M, 1.0 / self.M) if prior is None else np.asarray(prior, dtype=np.float64).reshape(-1)
        if w0.shape != (self.M,) or not np.isfinite(w0).all():
            raise ValueError(f"prior must hold {self.M} finite weights")
        st = self.pooled_stats(pool)
        G, Hs, _, Is = st.shape
        dev = st.device
        weight = torch.empty(G, Hs, self.M, Is, device=dev, dtype=torch.float64)
        intercept = torch.empty(G, Hs, Is, device=dev, dtype=torch.float64)
        status = torch.empty(G, Hs, Is, device=dev, dtype=torch.int32)
        dropped = torch.empty(G, Hs, Is, device=dev, dtype=torch.uint8)
        d = TecmCombineSolve(stats=st.data_ptr(), s_stride_g=st.stride(0), s_stride_h=st.stride(1), s_stride_k=st.stride(2),
                             s_stride_i=st.stride(3), G=G, H=Hs, I=Is, M=self.M, ridge=ridge,
                             weight=weight.data_ptr(), intercept=intercept.data_ptr(), status=status.data_ptr(),
                             dropped=dropped.data_ptr())
        for m in range(self.M):
            d.w0[m] = float(w0[m])
        check(lib().tecm_combine_solve(C.byref(d), stream_ptr()), "tecm_combine_solve")
        return Combination(weight.cpu().numpy(), intercept.cpu().numpy(), status.cpu().numpy(), dropped.cpu().numpy(),
                           st[:, :, 0, :].cpu().numpy(), st[:, :, self.K - 1, :].cpu().numpy(), self.member_names,
                           (self.H, self.I), ridge, pool, name, members)


class Combination:
    """A fitted combination.  numpy attributes, (G, H, N)-shaped with stride-0 axes where the fit was pooled: `weight`
    (G, H, M, N), `intercept`, `status` (bits EMPTY, FEW, DROPPED, NONFINITE), `dropped` (bit m: member m was dropped in
    that cell), `counts` and `skipped` (samples used / left out for a non-finite value); `member_names`, `ridge`, `pool`,
    `name` (its entry in the results when it is an element of `baselines=`).  `members` holds the member specs: the
    strings, and the fitted baseline objects, which `save` does not store."""

    def __init__(self, weight, intercept, status, dropped, counts, skipped, member_names, shape, ridge=0.0, pool="cell",
                 name=DEFAULT_NAME, members=None):
        self.member_names = [str(n) for n in member_names]
        self.M = len(self.member_names)
        self.H, self.N = int(shape[0]), int(shape[1])
        self._compact = dict(weight=np.ascontiguousarray(weight, dtype=np.float64),
                             intercept=np.ascontiguousarray(intercept, dtype=np.float64),
                             status=np.ascontiguousarray(status, dtype=np.int32),
                             dropped=np.ascontiguousarray(dropped, dtype=np.uint8),
                             counts=np.ascontiguousarray(counts, dtype=np.float64),
                             skipped=np.ascontiguousarray(skipped, dtype=np.float64))
        self.G = self._compact["weight"].shape[0]
        if self._compact["weight"].shape[2] != self.M:
            raise ValueError("weight must be (G, H, M, N)")
        self.weight = np.broadcast_to(self._compact["weight"], (self.G, self.H, self.M, self.N))
        for k in ("intercept", "status", "dropped", "counts", "skipped"):
            setattr(self, k, np.broadcast_to(self._compact[k], (self.G, self.H, self.N)))
        self.ridge, self.pool, self.name = float(ridge), str(pool), str(name)
        if not self.name or self.name == MODEL_NAME:
            raise ValueError(f"a combination needs a name other than {MODEL_NAME!r}")
        self.members = self._resolve(members)
        self._dev: Dict[str, tuple] = {}

    def _resolve(self, members) -> list:
        """Member specs in member order from a list of specs or a {name: object} dict; a baseline object that was not given
        stays None and raises when its forecast is needed."""
        if members is None:
            members = {}
        if not isinstance(members, dict):
            specs = list(members)
            if check_members(specs) != self.member_names:
                raise ValueError(f"members {check_members(specs)} do not match the fitted {self.member_names}")
            return specs
        out = []
        for n in self.member_names:
            if n == MODEL_MEMBER or n in KINDS:
                out.append(n)
            elif n in members:
                if member_name(members[n]) != n:
                    raise ValueError(f"member {n!r} was given a {member_name(members[n])!r}")
                out.append(members[n])
            else:
                out.append(None)
        return out

    # ------------------------------------------------------------------------------------------ files
    def save(self, path: str) -> str:
        """An `.npz` of arrays and strings only (the pooled axes at length 1)."""
        np.savez_compressed(path, **self._compact, member_names=np.array(self.member_names), shape=np.array([self.H, self.N]),
                            ridge=np.array(self.ridge), pool=np.array(self.pool), name=np.array(self.name))
        return path

    @classmethod
    def load(cls, path: str, members=None) -> "Combination":
        """`members`: {name: fitted baseline object} for the members that are objects ("SARIMA", "Linear"), or the full list
        of specs; string members need nothing."""
        with np.load(path, allow_pickle=False) as z:
            return cls(z["weight"], z["intercept"], z["status"], z["dropped"], z["counts"], z["skipped"],
                       [str(n) for n in z["member_names"]], [int(v) for v in z["shape"]], float(z["ridge"]), str(z["pool"]),
                       str(z["name"]), members)

    # ------------------------------------------------------------------------------------------ the blend
    def _coefficients(self, device):
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self._compact["weight"]).to(device), torch.from_numpy(self._compact["intercept"]).to(device))
        return self._dev[key]

    def combine(self, preds: Dict[str, torch.Tensor], groups: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The blend of one batch: `preds[name]` is member `name`'s (B, L_out, N[, 1]) float32 forecast on the device, any
        strides; `groups` (B,) int32 when the fit has more than one group.  Returns (B, L_out, N, 1) float32 (`out`, a
        (B, L_out, N) tensor with any strides, when given).  One launch of `tecm_combine_apply`."""
        missing = [n for n in self.member_names if n not in preds]
        if missing:
            raise ValueError(f"combine() needs a forecast of every member; missing {missing}")
        d = TecmCombineApply(H=self.H, G=self.G, I=self.N, M=self.M)
        keep, S = [], None
        for m, n in enumerate(self.member_names):
            p, S2, H2, I2, ps, ph, pi = _operand(preds[n], n)
            S = S2 if S is None else S
            if (S2, H2, I2) != (S, self.H, self.N):
                raise ValueError(f"shape mismatch: member {n} {tuple(preds[n].shape)}, horizons {self.H}, nodes {self.N}")
            keep.append(p)
            _fill(d.member[m], p, (ps, ph, pi))
        dev = keep[0].device
        w, b = self._coefficients(dev)
        pooled_h, pooled_i = w.shape[1] == 1 and self.H > 1, w.shape[3] == 1 and self.N > 1
        d.S = S
        d.weight, d.intercept = w.data_ptr(), b.data_ptr()
        d.w_stride_g, d.w_stride_h, d.w_stride_m, d.w_stride_i = (w.stride(0), 0 if pooled_h else w.stride(1), w.stride(2),
                                                                  0 if pooled_i else w.stride(3))
        d.b_stride_g, d.b_stride_h, d.b_stride_i = b.stride(0), 0 if pooled_h else b.stride(1), 0 if pooled_i else b.stride(2)
        if out is None:
            out = torch.empty(S, self.H, self.N, device=dev, dtype=torch.float32)
        else:
            _lib.require_gpu_tensor(out, "out")
            if out.shape != (S, self.H, self.N):
                raise ValueError(f"out must be {(S, self.H, self.N)}, got {tuple(out.shape)}")
        d.out, d.o_stride_s, d.o_stride_h, d.o_stride_i = out.data_ptr(), out.stride(0), out.stride(1), out.stride(2)
        ids = _group_ids(groups, S, self.G) if self.G > 1 else None
        errs = error_word(dev)
        d.group, d.err_flag = _lib.ptr(ids), errs.ptr()
        check(lib().tecm_combine_apply(C.byref(d), stream_ptr()), "tecm_combine_apply")
        if ids is not None:
            errs.post()
        return out.unsqueeze(-1)

    def _check_groups(self, groups, num_groups, where: str) -> None:
        if self.G > 1 and (groups is None or num_groups is None or int(num_groups) != self.G):
            raise ValueError(f"{self.name}: fitted with {self.G} groups, so {where} needs groups= and num_groups={self.G}")

    def _member_forecasts(self, dataset, indices, out, computed=()) -> Dict[str, torch.Tensor]:
        """{member name: forecast} for the windows `indices`: the model's output `out`, members found in `computed` (pairs of
        (element of `baselines=`, its forecast)) and, computed here, every other one."""
        preds = {}
        for n, spec in zip(self.member_names, self.members):
            if n == MODEL_MEMBER:
                if out is None:
                    raise ValueError(f"{self.name}: member {MODEL_MEMBER!r} needs the model's output")
                preds[n] = out
                continue
            if spec is None:
                raise ValueError(f"{self.name}: member {n!r} is a fitted baseline object; pass it again (members={{{n!r}: ...}})")
            found = [p for k, p in computed if (k == spec if isinstance(spec, str) and isinstance(k, str) else k is spec)]
            preds[n] = found[0] if found else baseline_forecast(dataset, indices, spec)
        return preds

    def forecast_batch(self, dataset, indices, out, ids=None, computed=()) -> torch.Tensor:
        """The blend for the windows `indices` of `dataset` given the model's output `out` for them (the form the scoring
        passes use)."""
        return self.combine(self._member_forecasts(dataset, indices, out, computed), ids)

    @torch.no_grad()
    def forecast(self, model, x, tf, edge_index, dataset, indices, edge_weight=None, groups=None) -> torch.Tensor:
        """The combined (B, L_out, N, 1) forecast for the windows `indices` of `dataset`, whose inputs are `x` and `tf`
        (`dataset.batch(indices)`); the model runs only when it is a member.  `groups`: (B,) int32 ids of these windows."""
        out = None
        if MODEL_MEMBER in self.member_names:
            model.eval()
            out = model(x, tf, edge_index, edge_weight)
        return self.forecast_batch(dataset, indices, out, groups)


@torch.no_grad()
def fit_combination(model, dataset, edge_index, batch_size, members=(MODEL_MEMBER, "mean", "last"), groups=None,
                    num_groups: int = 1, ridge: float = 0.0, prior=None, pool: str = "cell", name: str = DEFAULT_NAME,
                    edge_weight=None, order=None, group=None) -> Combination:
    """Fit a `Combination` of `members` on `dataset`, a HELD-OUT split (not the one the model was trained on, and not the one
    the combination is scored on): one `eval()` no-grad pass, the scoring pass of `evaluate_split` with one more launch per
    batch (`tecm_combine_moments`) and no host synchronisation, then one solve.

    `members`: "model", the kind strings of `window_baseline`, fitted `SarimaBaseline` / `LinearBaseline` / `AnalogBaseline`
    objects; at most 8, with unique names.  `groups` (one int32 id per dataset index, on the device) and `num_groups` fit one set of
    coefficients per group, as `evaluate_maps` stratifies its scores.  `ridge`, `prior`, `pool` as in
    `CombinationMoments.fit`; `order` and `group` as in `evaluate_split` (the moments are summed over the ranks)."""
    specs = list(members)
    names = check_members(specs)
    if pool not in POOLS:
        raise ValueError(f"pool must be one of {POOLS}, got {pool!r}")
    G = int(num_groups)
    if groups is not None and (groups.dtype != torch.int32 or groups.shape != (len(dataset),)):
        raise ValueError(f"groups must be an int32 tensor with one id per dataset index ({len(dataset)})")
    if G > 1 and groups is None:
        raise ValueError(f"{G} groups need groups=")
    plain = [s for s in specs if not (isinstance(s, str) and s == MODEL_MEMBER)]
    entry = {n: (MODEL_NAME if n == MODEL_MEMBER else baseline_name(s)) for n, s in zip(names, specs)}
    state: dict = {"cm": None, "preds": {}, "chunk": None}

    def per_forecast(fname, pred, y, chunk):
        state["preds"][fname] = pred
        state["chunk"] = chunk

    def per_batch(ordinal, x, tf, y, out, ids):
        if state["cm"] is None:
            state["cm"] = CombinationMoments(names, out.shape[1], out.shape[2], G, device=out.device)
        if groups is not None:
            ids = groups[torch.as_tensor(state["chunk"], dtype=torch.int64).to(groups.device, non_blocking=True)]
        state["cm"].update([state["preds"][entry[n]] for n in names], y, ids)
        state["preds"] = {}

    _score_pass(model, dataset, edge_index, batch_size, None, plain, edge_weight, order, None, None, per_batch=per_batch,
                per_forecast=per_forecast)
    cm = state["cm"]
    if cm is None:
        raise ValueError("fit_combination() on an empty dataset")
    cm.merge_(group)
    check_device_errors(cm.stats.device)
    return cm.fit(ridge, prior, pool, name, specs)


def write_combination(comb: Combination, output_dir: str, grid: Optional[Sequence[int]] = None) -> Dict[str, str]:
    """`combination_maps.npz`: `weight` (G, H, M, N) -- (G, H, M, *grid) when `grid`, e.g. (41, 71), is given --, `intercept`,
    `status`, `dropped`, `counts` and `member_names`; `combination_by_horizon.csv`: per group and horizon the mean weight of
    every member and the mean intercept over the nodes, the cells that dropped a member and the cells on a fallback (EMPTY,
    FEW or NONFINITE: the prior weights).  numpy and the standard library only.  Returns the two paths."""
    os.makedirs(output_dir, exist_ok=True)
    arrays = {}
    for k in ("weight", "intercept", "status", "dropped", "counts"):
        a = np.ascontiguousarray(getattr(comb, k))
        if grid is not None:
            check_grid(grid, a.shape[-1])
            a = a.reshape(*a.shape[:-1], *[int(d) for d in grid])
        arrays[k] = a
    arrays["member_names"] = np.array(comb.member_names)
    npz_path = os.path.join(output_dir, "combination_maps.npz")
    np.savez_compressed(npz_path, **arrays)
    csv_path = os.path.join(output_dir, "combination_by_horizon.csv")
    fallback = (comb.status & (EMPTY | FEW | NONFINITE)) != 0
    with open(csv_path, "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow(["group", "horizon"] + [f"weight_{n}" for n in comb.member_names] + ["intercept", "cells_dropped", "cells_fallback"])
        for g in range(comb.G):
            for h in range(comb.H):
                wr.writerow([g, h] + [repr(float(comb.weight[g, h, m].mean())) for m in range(comb.M)]
                            + [repr(float(comb.intercept[g, h].mean())), int((comb.dropped[g, h] != 0).sum()), int(fallback[g, h].sum())])
    return {"npz": npz_path, "csv": csv_path}
