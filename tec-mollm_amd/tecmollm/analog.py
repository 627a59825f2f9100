"""The analog ensemble as a probabilistic forecast: the K outcomes that followed the K nearest stretches of the training
record (`src.models.baselines.AnalogBaseline`) are an ensemble whose spread comes from the data, not from dropout masks.
`evaluate_analog_ensemble` scores them with the statistics `evaluate_ensemble` applies to MC-dropout members
(`EnsembleMetrics`: CRPS, spread / skill, rank histogram, coverage) and their mean like any other forecast, under the name
"Analog".  No model is involved: one `tecm_analog_search` and one `tecm_analog_forecast` launch per batch, the latter writing
the members and the mean together.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .devcheck import check_device_errors
from .evaluate import ANALOG_NAME, baseline_name
from .loop import _batches


@torch.no_grad()
def evaluate_analog_ensemble(analog, dataset, batch_size: int, scaler=None, trim: int = 1, groups: Optional[torch.Tensor] = None,
                             num_groups: int = 1, condition=None, order: Optional[Sequence[int]] = None,
                             fields=None, reorder=None):
    """Returns (results, maps, prob) as `evaluate_ensemble` does, with the single forecast "Analog": `results["Analog"]` is the
    `evaluate_horizons` dict of the members' mean -- bit for bit the entry `evaluate_split` gives the same fitted baseline at
    the same batch size --, `maps["Analog"]` its `MapMetrics.compute()`, and `prob` the `EnsembleMetrics.compute()` of the K
    members, which `write_ensemble` takes unchanged.  `groups` / `num_groups` as in `evaluate_maps`; `condition` as in
    `AnalogBaseline.search_windows`.  `fields` (a `tecmollm.fields.FieldSpec`) as in `evaluate_ensemble`: the members also
    feed a `FieldMetrics`, whose keys are added to `prob` -- the analog members are matched per node, so this is where their
    maps are judged; every other entry stays bit for bit the same.
    `reorder` (a `tecmollm.coherence.SchaakeTemplate`, or an `EccTemplate` built with its `edge_index`): the members of every
    batch are reordered in place by the template before they are scored, which makes maps of them.  The mean forecast is
    taken before that, and the per-cell scores sort each cell's members: `results`, `maps` and every per-cell entry of
    `prob` stay bit for bit the same, the field entries change.  None: nothing is reordered.

    Every cell must have found its K analogs: a cell with fewer would put NaN members into the scores, so the pass keeps
    one flag on the device, reads it once at the end and raises ValueError if it is set (lower `k`, drop a condition, or
    fit on a longer record)."""
    from src.evaluation.metrics import EnsembleMetrics, HorizonMetrics, MapMetrics
    from src.models.baselines import analog_forecast
    if baseline_name(analog) != ANALOG_NAME:
        raise ValueError("evaluate_analog_ensemble() needs a fitted AnalogBaseline")
    if groups is not None and (groups.dtype != torch.int32 or groups.shape != (len(dataset),)):
        raise ValueError(f"groups must be an int32 tensor with one id per dataset index ({len(dataset)})")
    hm = mm = em = fm = short = None
    for ordinal, chunk in enumerate(_batches(len(dataset), batch_size, order)):
        y = dataset.batch(chunk)[2]
        idx, _, count = analog.search_windows(dataset, chunk, condition)
        mean, members = analog_forecast(analog._Y_dev, idx, count, analog.match_len_, analog.H_, want_members=True)
        if em is None:
            H, N = mean.shape[1], mean.shape[2]
            hm = HorizonMetrics(H, scaler, device=mean.device)
            mm = MapMetrics(H, N, int(num_groups), scaler, device=mean.device)
            em = EnsembleMetrics(H, N, analog.k, int(num_groups), scaler, trim, device=mean.device)
            if fields is not None:
                fm = fields.metrics(H, N, analog.k, int(num_groups), scaler, mean.device)
            short = torch.zeros((), device=mean.device, dtype=torch.bool)
        short |= (count < analog.k).any()
        if reorder is not None:
            reorder.apply_(members, dataset, chunk, chunk=ordinal)
        ids = None
        if groups is not None:
            ids = groups[torch.as_tensor(chunk, dtype=torch.int64).to(groups.device, non_blocking=True)]
        em.update(members, y, ids)
        if fm is not None:
            fm.update(members, y, ids)
        pred = mean.unsqueeze(-1)
        hm.update(pred, y)
        mm.update(pred, y, ids)
    if em is None:
        raise ValueError("evaluate_analog_ensemble() on an empty dataset")
    if bool(short.item()):
        raise ValueError(f"some (window, node) found fewer than k = {analog.k} admitted analogs: its members would be NaN")
    results = {ANALOG_NAME: hm.merge_(None).compute()}
    maps = {ANALOG_NAME: mm.merge_(None).compute()}
    prob = em.merge_(None).compute()
    if fm is not None:
        prob.update(fields.entries(fm.merge_(None).compute()))
    check_device_errors(em.stats.device)
    return results, maps, prob
