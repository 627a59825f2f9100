"""Coherent ensemble maps: reorder the members of an ensemble so that each one is a map.

Two ensembles of this package have good margins and no spatial structure: the analog ensemble is matched per node (member k
at node i and member k at node j come from unrelated dates), and a quantile model emits calibrated levels per cell and no
members at all.  The per-cell scores (`EnsembleMetrics`) cannot see this, the field scores (`FieldMetrics`) can.  The standard
remedy is a reordering: in every cell keep the values, and hand them to the member indices in the rank order of a dependence
template whose members are real maps --

  * ensemble copula coupling (ECC; Schefzik, Thorarinsdottir and Gneiting 2013): the template is a raw ensemble, here the
    MC-dropout members of `ensemble_members` (`EccTemplate`);
  * the Schaake shuffle (Clark et al. 2004): the template is K observed maps of past dates from the training record
    (`SchaakeTemplate`), read from the record where it lies.

`reorder_members` is the kernel call (`tecm_member_reorder`, include/tecmollm.h (3n)); `quantile_members` turns quantile
levels into K equally likely members; `evaluate_quantile_ensemble` scores a quantile model as an ensemble of maps;
`evaluate_analog_ensemble(..., reorder=)` and `AnalogBaseline.members(..., reorder=)` take a template too.  The margins stay bit
for bit the same, so every per-cell score is unchanged; the rank structure across nodes (and, with dated rows, across
horizons) is borrowed from the template.

What it is not: ties in the template are broken by member index, not at random; the Schaake dates are drawn by time-of-day
slot only, not conditioned on the forecast or on the state of the ionosphere; the template needs exactly K members;
coherence across horizons comes only from the dated template, whose rows + h are consecutive maps -- not from ECC, whose
members draw independent dropout masks per forward.
"""
from __future__ import annotations

import weakref
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .devcheck import check_device_errors, error_word
from .evaluate import MODEL_NAME, _score_pass
from .functions import quantile_levels
from .loop import _batches


# ------------------------------------------------------------------------------------ the kernel call
def _khsn(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dim() == 5 and t.shape[-1] == 1:
        t = t.squeeze(-1)
    if t.dim() != 4:
        raise ValueError(f"{name} must be (K, S, H, N) or (K, S, H, N, 1), got {tuple(t.shape)}")
    return t


def _span(t: torch.Tensor):
    """The byte range [lo, hi) the view can touch."""
    lo = hi = 0
    for n, st in zip(t.shape, t.stride()):
        reach = (n - 1) * st
        lo, hi = lo + min(reach, 0), hi + max(reach, 0)
    return t.data_ptr() + lo * t.element_size(), t.data_ptr() + (hi + 1) * t.element_size()


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    (alo, ahi), (blo, bhi) = _span(a), _span(b)
    return alo < bhi and blo < ahi


@torch.no_grad()
def reorder_members(values: torch.Tensor, template: torch.Tensor, *, rows: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, return_ranks: bool = False):
    """In every cell (s, h, n): `out[k]` = the value whose position among the cell's K `values` is the position of
    `template[k]` among the cell's K template values.  Positions follow one total order: numbers by <, equal numbers (-0.0
    equals +0.0) by member index, NaN after every number and NaNs among themselves by member index.  The output holds
    exactly the cell's input values, bit patterns included.

    values    (K, S, H, N) or (K, S, H, N, 1) float32 on the device, any strides (the stack of model-shaped outputs viewed
              as (K, S, H, N) is read in place); 2 <= K <= 64.
    template  a member tensor of the same logical shape, any strides (ECC); or, with `rows`, a 2-D (T, N) float32 series view
              of any strides -- `dataset.Ys.view(T, N)`, or `analog._Y_dev.t()` for the node-major archive -- whose rows
              `rows[s, k] + h` are the template (the Schaake shuffle; no (K, S, H, N) template is built).
    rows      (S, K) int32 on the device.  A sample with a row < 0 or a row + H > T gets NaN members (and rank 255), and
              `check_device_errors` raises TecmError naming TECM_BAD_ROW; nothing is read outside the series.
    out       None (a new contiguous tensor), `values` itself (in place), or a tensor of the values' shape that overlaps
              neither operand.
    Returns `out` -- shaped like `values` --, or (`out`, ranks) with `return_ranks`: ranks (K, S, H, N) uint8, the position
    of every template member."""
    from . import ops
    v = _khsn(values, "values")
    K, S, H, N = v.shape
    if not 2 <= K <= _lib.TECM_ENS_MAX_K:
        raise ValueError(f"members must lie in [2, {_lib.TECM_ENS_MAX_K}], got {K}")
    if min(S, H, N) < 1:
        raise ValueError(f"values must hold at least one sample, horizon and node, got {tuple(values.shape)}")
    if not v.is_cuda or v.dtype != torch.float32:
        raise ValueError(f"values must be a float32 tensor on the GPU, got {v.dtype} on {v.device}")
    if not isinstance(template, torch.Tensor) or template.device != v.device or template.dtype != torch.float32:
        raise ValueError(f"template must be a float32 tensor on {v.device}, got "
                         f"{getattr(template, 'dtype', type(template))} on {getattr(template, 'device', None)}")
    if rows is None:
        t = _khsn(template, "template")
        if t.shape != v.shape:
            raise ValueError(f"shape mismatch: values {tuple(values.shape)}, template {tuple(template.shape)}: the template "
                             f"needs exactly K = {K} members of the same samples, horizons and nodes")
    else:
        t = template
        if t.dim() != 2 or t.shape[1] != N or t.shape[0] < H:
            raise ValueError(f"with rows the template must be a (T, {N}) series with T >= {H}, got {tuple(template.shape)}")
        if not isinstance(rows, torch.Tensor) or rows.device != v.device or rows.dtype != torch.int32:
            raise ValueError(f"rows must be an int32 tensor on {v.device}")
        if rows.shape != (S, K):
            raise ValueError(f"rows must hold one date per (sample, member): {tuple(rows.shape)} for (S, K) = {(S, K)}")
        rows = rows.contiguous()
    if out is None:
        o, result = torch.empty((K, S, H, N), device=v.device, dtype=torch.float32), None
    else:
        if not isinstance(out, torch.Tensor) or out.device != v.device or out.dtype != torch.float32:
            raise ValueError(f"out must be a float32 tensor on {v.device}")
        o, result = _khsn(out, "out"), out
        if o.shape != v.shape:
            raise ValueError(f"shape mismatch: values {tuple(values.shape)}, out {tuple(out.shape)}")
        same = o.data_ptr() == v.data_ptr() and o.stride() == v.stride()
        if not same and _overlap(o, v):
            raise ValueError("out overlaps values without being the same view: pass out=values to reorder in place")
        if _overlap(o, t) or (rows is not None and _overlap(o, rows)):
            raise ValueError("out overlaps the template")
        if any(n > 1 and st == 0 for n, st in zip(o.shape, o.stride())):
            raise ValueError("out is an expanded view: its cells share storage")
    ranks = torch.empty((K, S, H, N), device=v.device, dtype=torch.uint8) if return_ranks else None
    errs = error_word(v.device)
    ops.member_reorder(v, t, o, rows, ranks, errs.ptr())
    if rows is not None:
        errs.post()                            # only a date can set the word here
    if result is None:
        result = o.unsqueeze(-1) if values.dim() == 5 else o
    return (result, ranks) if return_ranks else result


# ------------------------------------------------------------------------------------ templates
def _target_series(dataset):
    """The target-scaled (T, N) series behind a dataset, as `AnalogBaseline.fit` obtains it, and its first usable row."""
    if "Ys" in dataset.__dict__:
        return dataset.Ys.view(dataset.Ys.shape[0], -1), 0
    from src.models.baselines import rebuilt_target_series
    Y = dataset.Y
    return rebuilt_target_series(Y.view(Y.shape[0], -1, Y.shape[3])), 1          # row 0 is in no window's target: NaN


def schaake_candidates(num_rows: int, first_row: int, L_out: int, slots, slot, same_slot: bool) -> np.ndarray:
    """The rows that may serve as a Schaake date, ascending: `first_row <= r`, the L_out rows `r .. r + L_out - 1` inside
    the record of `num_rows` rows and, with `same_slot`, a known time-of-day slot equal to `slot`."""
    last = num_rows - int(L_out)
    if same_slot:
        last = min(last, len(slots) - 1)
    r = np.arange(int(first_row), max(last + 1, int(first_row)), dtype=np.int64)
    return r[np.asarray(slots)[r] == slot] if same_slot else r


def schaake_select(candidates: np.ndarray, k: int, min_gap: int, seed: int, window: int) -> np.ndarray:
    """`k` of `candidates`, pairwise at least `min_gap` rows apart: the candidates are put in the random order of
    `numpy.random.default_rng([seed, window]).permutation` and taken in that order, skipping one that lies nearer than
    `min_gap` to a date already taken.  Member j gets the j-th date taken.  ValueError when fewer than `k` can be had."""
    perm = np.random.default_rng([int(seed), int(window)]).permutation(np.asarray(candidates, dtype=np.int64))
    taken: list = []
    for r in perm.tolist():
        if all(abs(r - c) >= min_gap for c in taken):
            taken.append(r)
            if len(taken) == k:
                return np.asarray(taken, dtype=np.int32)
    raise ValueError(f"window {window}: only {len(taken)} of {len(perm)} candidate dates lie {min_gap} rows apart, "
                     f"{k} are needed (lower k or min_gap, or use a longer record)")


class SchaakeTemplate:
    """The dependence template of the Schaake shuffle: for every window, `k` dates of the training record whose observed maps
    (the L_out consecutive rows from each date on) order the members.

    `train_dataset` is a `SlidingWindowSamplerDataset` or `SeriesWindowDataset`; the template keeps a view of its
    target-scaled series (`series`, (T, N): `dataset.Ys`, or the series rebuilt from `dataset.Y`) and the time-of-day slot of
    every row (`time_features[:, 0]`).  Dates are drawn on the host: `k` distinct rows from
    `numpy.random.default_rng([seed, window index])`, each with its L_out rows inside the record, pairwise at least `min_gap`
    rows apart (None: L_out, so that no two members share a map) and, with `same_slot`, in the time-of-day slot of the
    window's first target row.  The same (seed, window index) gives the same dates whatever the batch size or order."""

    def __init__(self, train_dataset, k: int, seed: int = 0, same_slot: bool = True, min_gap: Optional[int] = None):
        self.k, self.seed, self.same_slot = int(k), int(seed), bool(same_slot)
        if not 2 <= self.k <= _lib.TECM_ENS_MAX_K:
            raise ValueError(f"k must lie in [2, {_lib.TECM_ENS_MAX_K}], got {k}")
        self.L_out = int(train_dataset.L_out)
        self.min_gap = self.L_out if min_gap is None else int(min_gap)
        if self.min_gap < 1:
            raise ValueError(f"min_gap must be at least 1 (the dates are distinct), got {min_gap}")
        self.series, self.first_row = _target_series(train_dataset)
        self.slots = train_dataset.time_features[:, 0].to(torch.int64).cpu().numpy()
        self._query = None                     # (weak reference to the last queried dataset, its slot column on the host)

    @property
    def num_rows(self) -> int:
        return int(self.series.shape[0])

    def _query_slots(self, dataset) -> np.ndarray:
        if self._query is None or self._query[0]() is not dataset:
            self._query = (weakref.ref(dataset), dataset.time_features[:, 0].to(torch.int64).cpu().numpy())
        return self._query[1]

    def dates(self, dataset, index: int) -> np.ndarray:
        """The (k,) int32 rows of `series` drawn for window `index` of `dataset` (host)."""
        index = int(index)
        if not 0 <= index < dataset.num_samples:
            raise IndexError(f"Index {index} is out of bounds for a dataset of size {dataset.num_samples}")
        slot = None
        if self.same_slot:
            tf, origin = self._query_slots(dataset), dataset.sample_indices[index] + dataset.L_in
            if origin >= len(tf):
                raise ValueError(f"window {index}: its first target row {origin} has no time feature")
            slot = int(tf[origin])
        cand = schaake_candidates(self.num_rows, self.first_row, self.L_out, self.slots, slot, self.same_slot)
        return schaake_select(cand, self.k, self.min_gap, self.seed, index)

    def rows(self, dataset, indices: Sequence[int]) -> torch.Tensor:
        """The (B, k) int32 tensor of dates of the windows `indices` of `dataset`, on the device of the series."""
        if int(dataset.L_out) != self.L_out:
            raise ValueError(f"L_out: the template was built for {self.L_out} horizons, the dataset has L_out = {dataset.L_out}")
        host = np.stack([self.dates(dataset, i) for i in indices]) if len(indices) else np.zeros((0, self.k), np.int32)
        return torch.from_numpy(host).to(self.series.device, non_blocking=True)

    def apply_(self, members: torch.Tensor, dataset, indices: Sequence[int], x=None, tf=None, edge_index=None,
               chunk: int = 0) -> torch.Tensor:
        """Reorders `members` (K, B, L_out, N) of the windows `indices` in place.  `x`, `tf`, `edge_index` and `chunk` are what
        `EccTemplate.apply_` needs; the dates depend on the window indices alone."""
        if members.shape[0] != self.k:
            raise ValueError(f"the template has {self.k} members, the ensemble {members.shape[0]}")
        return reorder_members(members, self.series, rows=self.rows(dataset, indices), out=members)


class EccTemplate:
    """The dependence template of ensemble copula coupling: the raw ensemble of `ensemble_members` -- `members` MC-dropout
    forwards of one model under the seeds of `evaluate_ensemble` (member k of batch `chunk` under `member_seed(seed, chunk,
    k)`), or one forward of each of a sequence of models.  `edge_index` / `edge_weight` are only needed where the caller has
    no graph to pass (`evaluate_analog_ensemble(..., reorder=)`)."""

    def __init__(self, model_or_models, members: Optional[int] = 16, seed: int = 0, edge_index: Optional[torch.Tensor] = None,
                 edge_weight: Optional[torch.Tensor] = None):
        from .ensemble import _member_count
        self.model, self.seed = model_or_models, int(seed)
        self.k = _member_count(model_or_models, members)
        self.edge_index, self.edge_weight = edge_index, edge_weight

    def members(self, x: torch.Tensor, tf: torch.Tensor, edge_index: torch.Tensor, chunk: int = 0) -> torch.Tensor:
        from .ensemble import ensemble_members
        return ensemble_members(self.model, x, tf, edge_index, self.k, self.seed, int(chunk), self.edge_weight)

    def apply_(self, members: torch.Tensor, dataset, indices: Sequence[int], x=None, tf=None, edge_index=None,
               chunk: int = 0) -> torch.Tensor:
        """Reorders `members` (K, B, L_out, N) of the windows `indices` in place; `chunk` is the batch's ordinal in its pass."""
        if members.shape[0] != self.k:
            raise ValueError(f"the template has {self.k} members, the ensemble {members.shape[0]}")
        edge_index = self.edge_index if edge_index is None else edge_index
        if edge_index is None:
            raise ValueError("an EccTemplate used without a graph needs edge_index= at construction")
        if x is None or tf is None:
            x, tf, _ = dataset.batch(indices)
        return reorder_members(members, self.members(x, tf, edge_index, chunk), out=members)


# ------------------------------------------------------------------------------------ members of a quantile forecast
@torch.no_grad()
def quantile_members(levels: torch.Tensor, taus, K: int) -> torch.Tensor:
    """(B, Q, H, N) levels of `QuantileModel.quantiles` at the probabilities `taus` -> (K, B, H, N) float32 members, member k
    the piecewise-linear quantile function at p_k = (k + 0.5) / K.

    The levels are sorted per cell first (as `evaluate_quantiles` sorts crossing levels).  With tau_j <= p_k < tau_{j+1}, in
    float64: lo + (hi - lo) * ((p_k - tau_j) / (tau_{j+1} - tau_j)), rounded to float32 once.  Outside [tau_0, tau_{Q-1}] the
    member is the outermost level: no tail is invented, so K larger than the levels resolve gives tied outer members.
    Members ascend with k in every cell -- the comonotone ensemble; `reorder_members` makes maps of it."""
    ts = quantile_levels(taus)
    K = int(K)
    if K < 1:
        raise ValueError(f"K must be positive, got {K}")
    if levels.dim() != 4 or levels.shape[1] != len(ts):
        raise ValueError(f"levels must be (B, Q = {len(ts)}, H, N), got {tuple(levels.shape)}")
    z = torch.sort(levels.to(torch.float64), dim=1).values
    out = torch.empty((K, levels.shape[0]) + tuple(levels.shape[2:]), device=levels.device, dtype=torch.float32)
    for k in range(K):
        p = (k + 0.5) / K
        if p <= ts[0]:
            out[k] = z[:, 0]
        elif p >= ts[-1]:
            out[k] = z[:, -1]
        else:
            j = max(n for n in range(len(ts) - 1) if ts[n] <= p)
            w = (p - ts[j]) / (ts[j + 1] - ts[j])
            out[k] = z[:, j] + (z[:, j + 1] - z[:, j]) * w
    return out


@torch.no_grad()
def evaluate_quantile_ensemble(qmodel, dataset, edge_index: torch.Tensor, batch_size: int, template, members: int = 16,
                               scaler=None, intervals=None, trim: int = 1, groups: Optional[torch.Tensor] = None,
                               num_groups: int = 1, fields=None, order: Optional[Sequence[int]] = None,
                               edge_weight: Optional[torch.Tensor] = None):
    """A quantile model scored as an ensemble of maps: returns (results, maps, prob) shaped like `evaluate_ensemble`'s.

    One `eval()` pass (`_score_pass`): `results` / `maps` hold "TEC-MoLLM", the tau = 0.5 level, exactly as `evaluate_split` /
    `evaluate_maps` score `qmodel`.  Per batch the levels of that same forward become `members` members (`quantile_members`),
    `template` -- a `SchaakeTemplate`, an `EccTemplate`, or None for the members in level order, the comonotone baseline --
    reorders them in place, and they feed an `EnsembleMetrics` (whose `compute()` is `prob`) and, with `fields` (a
    `tecmollm.fields.FieldSpec`), a `FieldMetrics` as in `evaluate_ensemble`.  The per-cell entries of `prob` do not depend on
    the template; the field entries do.
    `intervals` (a `CQRIntervals` of a pair (tau_lo, tau_hi)): the pair's levels are shifted by their calibrated offset before
    the interpolation, as `quantile_forecast` shifts them (the offset is divided by the scaler's scale: the members stay in
    scaled units; `scaler` must be the one the intervals were calibrated with).  `groups` / `num_groups` / `order` as in
    `evaluate_maps`."""
    from src.evaluation.metrics import EnsembleMetrics
    from .quantile import _check_groups, _intervals_fit, _scaler_clip
    _check_groups(groups, dataset)
    _intervals_fit(intervals, qmodel, num_groups)
    K = int(members)
    if template is not None and template.k != K:
        raise ValueError(f"the template has {template.k} members, members = {K}: the template needs exactly K members")
    chunks = list(_batches(len(dataset), batch_size, order))
    shift = None
    if intervals is not None:
        _, _, scale, _ = _scaler_clip(intervals.scaler)
        shift = torch.from_numpy(intervals.offset / np.float32(scale)).to(edge_index.device)          # (G, H, N), scaled units
    box: list = []

    def per_batch(ordinal, x, tf, y, out, ids):
        lv = qmodel.quantiles_of(out)                                      # (B, Q, H, N) view of this forward's output
        if not box:
            H, N = lv.shape[2], lv.shape[3]
            box.append(EnsembleMetrics(H, N, K, int(num_groups), scaler, trim, device=lv.device))
            box.append(None if fields is None else fields.metrics(H, N, K, int(num_groups), scaler, lv.device))
        if shift is not None:
            # (an id outside its range is skipped and reported by the statistics: any row of offsets will do for it)
            off = shift[ids.to(torch.int64).clamp_(0, shift.shape[0] - 1)] if (ids is not None and shift.shape[0] > 1) else shift[:1]
            lv = lv.clone()
            lv[:, intervals.lo_idx] -= off
            lv[:, intervals.hi_idx] += off
        mem = quantile_members(lv, qmodel.taus, K)
        if template is not None:
            template.apply_(mem, dataset, chunks[ordinal], x=x, tf=tf, edge_index=edge_index, chunk=ordinal)
        box[0].update(mem, y, ids)
        if box[1] is not None:
            box[1].update(mem, y, ids)

    hms, mms = _score_pass(qmodel, dataset, edge_index, batch_size, scaler, (), edge_weight, order, groups, int(num_groups),
                           per_batch)
    if not hms:
        raise ValueError("evaluate_quantile_ensemble() on an empty dataset")
    results = {MODEL_NAME: hms[MODEL_NAME].merge_(None).compute()}
    maps = {MODEL_NAME: mms[MODEL_NAME].merge_(None).compute()}
    prob = box[0].merge_(None).compute()
    if box[1] is not None:
        prob.update(fields.entries(box[1].merge_(None).compute()))
    check_device_errors(box[0].stats.device)
    return results, maps, prob
