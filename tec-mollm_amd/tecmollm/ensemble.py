"""Ensemble forecasts: K stochastic forwards of one trained model (Monte-Carlo dropout) or one forward of each of K
separately trained models (a deep ensemble), and what is made of the members -- a forecast with an error bar
(`ensemble_forecast`), proper probabilistic scores of a test split (`evaluate_ensemble`) and their files (`write_ensemble`).

The reference's `test.py` runs the model in `eval()` and pools everything into one number per horizon; it has no
counterpart.  Three things make this cheap here: the model's five dropout sites draw their masks from a counter-based hash
keyed by an explicit seed (`csrc/common.h`), so a training-mode forward under `dropout_seed` is reproducible member by
member; the no-grad forward keeps nothing across GPT-2 blocks, so K members cost K forwards and no extra memory; and the
members are scored where they lie (`tecm_ensemble_stats` under `EnsembleMetrics`), with no host copy.

A member is the model's raw output in the target scaler's units; `scaler` turns the scores into TECU as it does for
`evaluate_split`.
"""
from __future__ import annotations

import csv
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import ops
from .devcheck import check_device_errors
from .functions import dropout_seed
from .evaluate import MODEL_NAME, baseline_names, batch_forecasts, check_grid
from .loop import _batches

MC_NAME = "TEC-MoLLM-MC"
_CHUNK_BITS, _MEMBER_BITS = 56, 8


def member_seed(seed: int, chunk: int, k: int) -> int:
    """The dropout base seed (`DropPlan.base_seed`) of member `k` of batch number `chunk` of a run with seed `seed`:

        splitmix64((splitmix64(seed mod 2^64) + chunk * 256 + k) mod 2^64),     0 <= k < 256, 0 <= chunk < 2^56

    A pure function.  splitmix64 is a bijection of the 64-bit integers and `chunk * 256 + k` is a different 64-bit number
    for every pair in range, so for one `seed` no two (chunk, k) share a value: no two members of a run draw the same
    masks.  The result is a non-negative 64-bit integer, which `DropPlan.base_seed` takes as it is (each site's seed is
    splitmix64 of `base_seed * 1000003 + site`, reduced mod 2^64 there)."""
    chunk, k = int(chunk), int(k)
    if not 0 <= k < (1 << _MEMBER_BITS) or not 0 <= chunk < (1 << _CHUNK_BITS):
        raise ValueError(f"member_seed needs 0 <= k < {1 << _MEMBER_BITS} and 0 <= chunk < 2^{_CHUNK_BITS} (k {k}, chunk {chunk})")
    return ops.splitmix64(ops.splitmix64(int(seed) & ops._MASK64) + (chunk << _MEMBER_BITS) + k)


def _models(model_or_models) -> Optional[list]:
    """None for one model; the list for a sequence of them."""
    if isinstance(model_or_models, torch.nn.Module):
        return None
    models = list(model_or_models)
    if not models or not all(isinstance(m, torch.nn.Module) for m in models):
        raise ValueError("expected a model or a non-empty sequence of models")
    return models


def _member_count(model_or_models, members: Optional[int]) -> int:
    """K: `members` for one model; the number of models for a sequence of them (`members` is then ignored)."""
    models = _models(model_or_models)
    if models is not None:
        return len(models)
    if members is None or int(members) < 1:
        raise ValueError(f"members must be a positive number, got {members}")
    return int(members)


@torch.no_grad()
def ensemble_members(model_or_models, x: torch.Tensor, tf: torch.Tensor, edge_index: torch.Tensor,
                     members: Optional[int], seed: int, chunk: int = 0,
                     edge_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The members of an ensemble forecast of one batch: a (K, B, L_out, N) float32 device tensor, node-contiguous, of raw
    outputs in scaled units.

    One model: K = `members` training-mode forwards (every dropout site active), member k under
    `dropout_seed(member_seed(seed, chunk, k))` -- the same (seed, chunk) gives the same bits, and member k is the plain
    `model.train()` forward under that seed.  The model's `training` flag is put back afterwards, also when a forward
    raises.  A sequence of models (separately trained checkpoints): each runs once in `eval()` mode, one member per
    model; `members`, `seed` and `chunk` are then not used.
    Nothing is kept for a backward (no grad), so the forwards run the lean path whatever the training flag, and every
    member is one transposing copy of the model's permuted output."""
    models = _models(model_or_models)
    K = _member_count(model_or_models, members)
    out = None
    for k in range(K):
        model = model_or_models if models is None else models[k]
        was_training = model.training
        try:
            model.train(models is None)
            if models is None:
                with dropout_seed(member_seed(seed, chunk, k)):
                    y = model(x, tf, edge_index, edge_weight)
            else:
                y = model(x, tf, edge_index, edge_weight)
        finally:
            model.train(was_training)
        y = y.squeeze(-1)                                                  # (B, L_out, N) view of (B, N, L_out)
        if out is None:
            out = torch.empty((K,) + tuple(y.shape), device=y.device, dtype=torch.float32)
        elif y.shape != out.shape[1:]:
            raise ValueError(f"member {k} has shape {tuple(y.shape)}, member 0 {tuple(out.shape[1:])}")
        out[k].copy_(y)
    return out


@torch.no_grad()
def ensemble_forecast(model_or_models, x: torch.Tensor, tf: torch.Tensor, edge_index: torch.Tensor,
                      members: Optional[int] = 16, seed: int = 0, scaler=None, trim: int = 1,
                      edge_weight: Optional[torch.Tensor] = None) -> Dict[str, object]:
    """A forecast with its error bar: {"mean", "std", "lo", "hi"}, device tensors (B, L_out, N) in TECU (in scaled units
    without `scaler`) -- the ensemble mean, the members' standard deviation (K - 1 in the denominator) and the interval
    [x_(1+trim), x_(K-trim)] between the sorted members --, "members" (K, B, L_out, N), raw, and "nominal_coverage", the
    share (K - 2 trim - 1) / (K + 1) of truths that interval holds if members and truth are exchangeable.  With a
    sequence of models K is their number and `members` is not used."""
    from src.evaluation.metrics import EnsembleMetrics
    mem = ensemble_members(model_or_models, x, tf, edge_index, members, seed, 0, edge_weight)
    K, B, H, N = mem.shape
    em = EnsembleMetrics(H, N, K, 1, scaler, trim, device=mem.device)
    truth = torch.zeros(1, device=mem.device, dtype=torch.float32).expand(B, H, N)      # not used by what is returned
    out: Dict[str, object] = dict(em.update(mem, truth, None, outputs=("mean", "std", "lo", "hi")))
    out["members"] = mem
    out["nominal_coverage"] = em.nominal_coverage
    return out


@torch.no_grad()
def evaluate_ensemble(model_or_models, dataset, edge_index: torch.Tensor, batch_size: int,
                      members: Optional[int] = 16, seed: int = 0, scaler=None, trim: int = 1,
                      baselines: Sequence[str] = ("mean",), groups: Optional[torch.Tensor] = None, num_groups: int = 1,
                      edge_weight: Optional[torch.Tensor] = None, order: Optional[Sequence[int]] = None, group=None,
                      first_chunk: int = 0, fields=None):
    """`evaluate_maps` plus the ensemble: returns (results, maps, prob).

    One pass over the batches.  Per batch: the deterministic `eval()` forward and the baselines, scored exactly as
    `evaluate_split` / `evaluate_maps` score them (the same entries, key for key and bit for bit), then the K members with
    `chunk` = `first_chunk` + the batch's ordinal in this pass (a rank that scores a shard passes the number of batches
    before its own, so that no two batches of a run share their masks and the shards add up to the single pass).  The ensemble-mean forecast (`mean_raw` of the kernel, scaled units) is
    scored like any other forecast under the name "TEC-MoLLM-MC", the last entry of `results` and `maps`; the members feed an
    `EnsembleMetrics`, whose `compute()` is `prob`.  With a sequence of models the deterministic entry is the first model's.
    `groups`, `num_groups`, `order` and `group` as in `evaluate_maps`.
    `fields` (a `tecmollm.fields.FieldSpec`): the same members also feed a `FieldMetrics` -- the energy score and the variogram
    score, which see the members as maps --, whose `compute()` keys (its sample count as "field_count") and `FieldSpec.describe()`
    are added to `prob`; every other entry is bit for bit what the call without `fields` returns."""
    from src.evaluation.metrics import EnsembleMetrics, HorizonMetrics, MapMetrics
    if groups is not None and (groups.dtype != torch.int32 or groups.shape != (len(dataset),)):
        raise ValueError(f"groups must be an int32 tensor with one id per dataset index ({len(dataset)})")
    kinds = list(baselines)
    base_names = baseline_names(kinds, groups, num_groups, "evaluate_ensemble")
    models = _models(model_or_models)
    K = _member_count(model_or_models, members)
    first = model_or_models if models is None else models[0]
    names = [MODEL_NAME] + base_names + [MC_NAME]
    hms: Dict[str, HorizonMetrics] = {}
    mms: Dict[str, MapMetrics] = {}
    em = fm = None
    for ordinal, chunk in enumerate(_batches(len(dataset), batch_size, order)):
        x, tf, y = dataset.batch(chunk)
        first.eval()
        out = first(x, tf, edge_index, edge_weight)
        if em is None:
            H, N = out.shape[1], out.shape[2]
            for name in names:
                hms[name] = HorizonMetrics(H, scaler, device=out.device)
                mms[name] = MapMetrics(H, N, int(num_groups), scaler, device=out.device)
            em = EnsembleMetrics(H, N, K, int(num_groups), scaler, trim, device=out.device)
            if fields is not None:
                fm = fields.metrics(H, N, K, int(num_groups), scaler, out.device)
        ids = None
        if groups is not None:
            ids = groups[torch.as_tensor(chunk, dtype=torch.int64).to(groups.device, non_blocking=True)]
        mem = ensemble_members(model_or_models, x, tf, edge_index, members, seed, int(first_chunk) + ordinal, edge_weight)
        mean_raw = em.update(mem, y, ids, outputs=("mean_raw",))["mean_raw"]
        if fm is not None:
            fm.update(mem, y, ids)
        forecasts = batch_forecasts(dataset, chunk, out, base_names, kinds, ids)
        forecasts.append((MC_NAME, mean_raw.unsqueeze(-1)))
        for name, pred in forecasts:
            hms[name].update(pred, y)
            mms[name].update(pred, y, ids)
    if em is None:
        raise ValueError("evaluate_ensemble() on an empty dataset")
    results = {name: hm.merge_(group).compute() for name, hm in hms.items()}
    maps = {name: mm.merge_(group).compute() for name, mm in mms.items()}
    prob = em.merge_(group).compute()
    if fm is not None:
        prob.update(fields.entries(fm.merge_(group).compute()))
    check_device_errors(em.stats.device)
    return results, maps, prob


CSV_COLUMNS = ("crps", "fair_crps", "rmse_mean", "spread", "spread_skill", "coverage", "nominal_coverage", "interval_width")


def write_ensemble(prob: Dict[str, object], output_dir: str, grid: Optional[Sequence[int]] = None) -> Dict[str, str]:
    """The files of `evaluate_ensemble`'s third result: `ensemble_maps.npz` with one (G, H, N) array per key of
    `ENSEMBLE_KEYS` -- (G, H, *grid) when `grid`, e.g. (41, 71), is given -- plus `rank_histogram` (G, H, K+1) and
    `nominal_coverage`; and `ensemble_by_horizon.csv` with one row per group and horizon: the scores of that group's
    statistics pooled over the nodes (CSV_COLUMNS).  numpy and the standard library only.  Returns the two paths."""
    from src.evaluation.metrics import ENSEMBLE_KEYS
    os.makedirs(output_dir, exist_ok=True)
    arrays = {}
    for k in ENSEMBLE_KEYS:
        a = np.asarray(prob[k])
        if grid is not None:
            check_grid(grid, a.shape[2])
            a = a.reshape(a.shape[0], a.shape[1], *[int(d) for d in grid])
        arrays[k] = a
    arrays["rank_histogram"] = np.asarray(prob["rank_histogram"])
    arrays["nominal_coverage"] = np.asarray(float(prob["nominal_coverage"]))
    npz_path = os.path.join(output_dir, "ensemble_maps.npz")
    np.savez_compressed(npz_path, **arrays)
    csv_path = os.path.join(output_dir, "ensemble_by_horizon.csv")
    with open(csv_path, "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow(["group", "horizon"] + list(CSV_COLUMNS))
        for g, pooled in enumerate(prob["by_group"]):
            for h in range(len(pooled["crps_by_horizon"])):
                wr.writerow([g, h] + [repr(float(prob["nominal_coverage"] if k == "nominal_coverage"
                                                 else pooled[f"{k}_by_horizon"][h])) for k in CSV_COLUMNS])
    return {"npz": npz_path, "csv": csv_path}
