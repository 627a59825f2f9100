"""Event verification of a test split on the device: did the model forecast the event?

The other evaluation passes answer "how large is the error" (`evaluate_split`, `evaluate_maps`, `evaluate_ensemble`,
`evaluate_conformal`, `evaluate_significance`).  A space-weather forecaster asks first whether a storm enhancement was hit,
missed or falsely announced -- TEC above 40 TECU over a cell, a positive storm phase (TEC more than 30 % above the quiet-time
value of that cell and hour), a negative phase (30 % below) -- and RMSE or CRPS do not say; they also punish a crest forecast
one cell too far south twice (the "double penalty").  This module adds the standard categorical complement:

  * `EventThresholds`: absolute thresholds in TECU, or thresholds relative to a per-(node, time-of-day slot) climatology such
    as `HistoricalAverage.averages`;
  * `target_slots`: the time-of-day slot of every target step of a batch, on the device;
  * `evaluate_events`: `evaluate_split`'s single pass plus, per forecast, contingency tables with POD / FAR / POFD / CSI /
    ETS / HSS / frequency bias per (group, threshold, horizon, node) and pooled, the fractions skill score over
    neighbourhoods of the grid, and for the MC-dropout ensemble the Brier score with its decomposition, the reliability
    diagram and the ROC -- all from integer counts kept on the device (`tecm_event_hist`, `tecm_event_fss` under
    `EventMetrics`), with no host copy of any forecast;
  * `write_events`: the files.

The reference has no counterpart.  Not covered: neighbourhood probabilities of the members for the FSS, thresholds from
quantiles of the data, plots.
"""
from __future__ import annotations

import csv
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .devcheck import check_device_errors
from .evaluate import _score_pass, check_grid

MC_NAME = "TEC-MoLLM-MC"
NUM_SLOTS = 12            # two-hourly time-of-day slots (column 0 of the time features)


class EventThresholds:
    """Q thresholds with a direction each.  `values` is a float32 numpy array addressed as
    values.flat[q*strides[0] + slot*strides[1] + node*strides[2]] (element strides, any of which may be 0): (Q,) with strides
    (1, 0, 0) for absolute thresholds, (Q, 12, N) with strides (12 N, N, 1) for climatology-relative ones.  `dirs[q]` is +1
    (the event is value > threshold) or -1 (value < threshold); the comparison is strict and in float32."""

    def __init__(self, values: np.ndarray, strides: Sequence[int], dirs: Sequence[int], labels: Sequence[str],
                 num_slots: int = 1, num_nodes: Optional[int] = None):
        self.values = np.ascontiguousarray(values, dtype=np.float32)
        self.strides = tuple(int(s) for s in strides)
        self.dirs = [1 if int(d) > 0 else -1 for d in dirs]
        self.labels = [str(s) for s in labels]
        self.num_slots, self.num_nodes = int(num_slots), (None if num_nodes is None else int(num_nodes))
        if len(self.strides) != 3 or min(self.strides) < 0:
            raise ValueError(f"strides must be three non-negative element strides, got {strides}")
        if any(int(d) == 0 for d in dirs) or len(self.dirs) != len(self.labels) or not self.dirs:
            raise ValueError("one non-zero direction and one label per threshold")
        last = (self.Q - 1) * self.strides[0] + (self.num_slots - 1) * self.strides[1] + ((self.num_nodes or 1) - 1) * self.strides[2]
        if self.num_slots < 1 or last >= self.values.size:
            raise ValueError(f"values of size {self.values.size} do not hold index {last}")
        self._tensors: Dict[str, torch.Tensor] = {}

    @property
    def Q(self) -> int:
        return len(self.dirs)

    @classmethod
    def absolute(cls, values, below=False, labels=None) -> "EventThresholds":
        """Thresholds in TECU, the same for every node and hour.  `below` (one bool, or one per value) turns the event into
        value < threshold."""
        v = np.asarray(values, dtype=np.float32).reshape(-1)
        b = np.broadcast_to(np.asarray(below, dtype=bool), v.shape)
        if labels is None:
            labels = [f"{'<' if lo else '>'} {float(x):g} TECU" for x, lo in zip(v, b)]
        return cls(v, (1, 0, 0), [-1 if lo else 1 for lo in b], labels)

    @classmethod
    def relative(cls, climatology, rel=(+0.3, -0.3)) -> "EventThresholds":
        """Thresholds relative to a climatology (N, 12) in TECU, such as `HistoricalAverage.averages`: t[q, slot, node] =
        clim[node, slot] * (1 + rel[q]), formed in float64 and rounded to float32 once; the event is value > t for rel >= 0
        (a positive phase) and value < t for rel < 0 (a negative phase)."""
        clim = np.asarray(climatology, dtype=np.float64)
        if clim.ndim != 2 or clim.shape[1] != NUM_SLOTS:
            raise ValueError(f"climatology must be (N, {NUM_SLOTS}), got {clim.shape}")
        rel = [float(r) for r in np.asarray(rel, dtype=np.float64).reshape(-1)]
        N = clim.shape[0]
        table = np.stack([clim.T * (1.0 + r) for r in rel]).astype(np.float32)          # (Q, 12, N)
        labels = [f"{'<' if r < 0 else '>'} {r:+.0%} of climatology" for r in rel]
        return cls(table, (NUM_SLOTS * N, N, 1), [-1 if r < 0 else 1 for r in rel], labels, NUM_SLOTS, N)

    def tensor(self, device) -> torch.Tensor:
        """The values as a contiguous float32 tensor on `device` (uploaded once per device)."""
        key = str(torch.device(device))
        if key not in self._tensors:
            self._tensors[key] = torch.from_numpy(self.values).to(device).contiguous()
        return self._tensors[key]

    def at(self, q: int, slot: int = 0, node: int = 0) -> float:
        """The threshold the kernels read for (q, slot, node)."""
        return float(self.values.reshape(-1)[q * self.strides[0] + slot * self.strides[1] + node * self.strides[2]])

    def save(self, path: str) -> str:
        """An `.npz` of arrays: values, strides, dirs, labels, num_slots, num_nodes (-1: any)."""
        np.savez(path, values=self.values, strides=np.asarray(self.strides, dtype=np.int64),
                 dirs=np.asarray(self.dirs, dtype=np.int32), labels=np.asarray(self.labels, dtype=np.str_),
                 num_slots=np.int64(self.num_slots), num_nodes=np.int64(-1 if self.num_nodes is None else self.num_nodes))
        return path if path.endswith(".npz") else path + ".npz"

    @classmethod
    def load(cls, path: str) -> "EventThresholds":
        with np.load(path, allow_pickle=False) as z:
            nodes = int(z["num_nodes"])
            return cls(z["values"], z["strides"].tolist(), z["dirs"].tolist(), [str(s) for s in z["labels"]],
                       int(z["num_slots"]), None if nodes < 0 else nodes)


def target_slots(dataset, indices: Sequence[int]) -> torch.Tensor:
    """(B, L_out) int32 on the device: the time-of-day slot of every target step of the windows `indices`,
    time_features[start + L_in + h, 0], for `SlidingWindowSamplerDataset` and `SeriesWindowDataset` alike.  The starts go up
    with a non-blocking copy and the gather runs on the device: no host synchronisation."""
    idx = [int(i) for i in indices]
    for i in idx:
        if not 0 <= i < dataset.num_samples:
            raise IndexError(f"Index {i} is out of bounds for a dataset of size {dataset.num_samples}")
    tf = dataset.time_features
    host = torch.tensor([dataset.sample_indices[i] + dataset.L_in for i in idx], dtype=torch.int64)
    if idx and int(host.max()) + dataset.L_out > tf.shape[0]:
        raise IndexError("the time features end before the last target step")
    first = host.to(tf.device, non_blocking=True)
    rows = first[:, None] + torch.arange(dataset.L_out, device=tf.device, dtype=torch.int64)[None, :]
    return tf[:, 0][rows].to(torch.int32)


@torch.no_grad()
def evaluate_events(model_or_models, dataset, edge_index: torch.Tensor, batch_size: int, thresholds: EventThresholds,
                    scaler=None, baselines: Sequence[str] = ("mean",), groups: Optional[torch.Tensor] = None,
                    num_groups: int = 1, members: Optional[int] = None, seed: int = 0, grid=None, scales=(1, 3, 5, 9),
                    edge_weight: Optional[torch.Tensor] = None, order: Optional[Sequence[int]] = None, group=None,
                    first_chunk: int = 0):
    """`evaluate_split` plus event verification: returns (results, events) with `results` exactly what `evaluate_split`
    returns and `events[name]` the `EventMetrics.compute()` dict (members = 1; with `grid` = (rows, cols) the FSS over the
    window widths `scales` too) of the model and of every baseline, fitted `SarimaBaseline` / `LinearBaseline` objects
    included.

    With `members=K` (or a sequence of models) there is also an entry "TEC-MoLLM-MC": its probabilistic scores (Brier and its
    decomposition, reliability, ROC) come from the K members, drawn with `ensemble_members(..., seed, first_chunk + ordinal)`
    exactly as `evaluate_ensemble` draws them; its categorical scores and FSS from the ensemble-mean forecast (`mean_raw` of
    `EnsembleMetrics.update`).  `groups` holds one int32 id in [0, num_groups) per DATASET index (`window_groups_by_index`);
    the slot of every target step comes from the dataset's time features (`target_slots`) when the thresholds depend on it.
    One pass, no host synchronisation inside it; `check_device_errors` runs at the end.  `order`, `group` and `first_chunk`
    as in `evaluate_ensemble`: shards add up to the single pass exactly, the counts being integers."""
    from src.evaluation.metrics import EnsembleMetrics, EventMetrics, EVENT_PROBABILISTIC_KEYS
    from .ensemble import _member_count, _models, ensemble_members
    if groups is not None and (groups.dtype != torch.int32 or groups.shape != (len(dataset),)):
        raise ValueError(f"groups must be an int32 tensor with one id per dataset index ({len(dataset)})")
    models = _models(model_or_models)
    first = model_or_models if models is None else models[0]
    with_mc = members is not None or models is not None
    K = _member_count(model_or_models, members) if with_mc else 0
    if with_mc and K < 2:
        raise ValueError(f"the ensemble entry needs at least 2 members, got {K}")
    ems: Dict[str, EventMetrics] = {}
    state = {"chunk": None, "ids": None, "slots": None, "prob": None, "mean": None}

    def make(out, k=1, with_grid=True):
        return EventMetrics(out.shape[1], out.shape[2], thresholds, int(num_groups), scaler, k,
                            grid if with_grid else None, scales, device=out.device)

    def per_forecast(name, pred, y, chunk):
        if state["chunk"] is not chunk:                                    # the first forecast of a batch
            state["chunk"] = chunk
            state["ids"] = None if groups is None else \
                groups[torch.as_tensor(chunk, dtype=torch.int64).to(groups.device, non_blocking=True)]
            state["slots"] = target_slots(dataset, chunk) if thresholds.num_slots > 1 else None
        if name not in ems:
            ems[name] = make(pred)
        ems[name].update(pred, y, state["ids"], state["slots"])

    def per_batch(ordinal, x, tf, y, out, ids):
        if not with_mc:
            return
        mem = ensemble_members(model_or_models, x, tf, edge_index, members, seed, int(first_chunk) + ordinal, edge_weight)
        if state["prob"] is None:
            state["prob"] = make(out, K, False)
            state["mean"] = EnsembleMetrics(out.shape[1], out.shape[2], K, 1, scaler, 0, device=out.device)
            ems[MC_NAME] = make(out)
        state["prob"].update(mem, y, state["ids"], state["slots"])
        state["mean"].reset()
        mean_raw = state["mean"].update(mem, y, None, outputs=("mean_raw",))["mean_raw"]
        ems[MC_NAME].update(mean_raw.unsqueeze(-1), y, state["ids"], state["slots"])

    hms, _ = _score_pass(first, dataset, edge_index, batch_size, scaler, baselines, edge_weight, order, None, None,
                         per_batch=per_batch, per_forecast=per_forecast)
    if not hms:
        raise ValueError("evaluate_events() on an empty dataset")
    results = {name: hm.merge_(group).compute() for name, hm in hms.items()}
    events = {name: em.merge_(group).compute() for name, em in ems.items()}
    if with_mc:
        prob = state["prob"].merge_(group).compute()
        keep = [k for k in prob if k.split("_pooled")[0].split("_all")[0] in EVENT_PROBABILISTIC_KEYS]
        for k in keep + ["reliability", "roc_curve"]:
            events[MC_NAME][k] = prob[k]
        events[MC_NAME]["members"] = K
    check_device_errors(next(iter(ems.values())).hist.device)
    return results, events


POOLED_COLUMNS = ("base_rate", "pod", "far", "pofd", "csi", "ets", "hss", "frequency_bias")
PROB_COLUMNS = ("brier", "brier_reliability", "brier_resolution", "brier_uncertainty", "brier_skill", "roc_area")


def write_events(events: Dict[str, Dict[str, object]], output_dir: str, grid: Optional[Sequence[int]] = None) -> Dict[str, str]:
    """The files of `evaluate_events`' second result: `event_maps.npz` with one array `<forecast>/<score>` of shape (G, Q, H, N)
    per forecast and per-node score -- (G, Q, H, *grid) when `grid` is given -- plus `<forecast>/table` (G, Q, H, 4, N);
    `event_scores.csv` with one row per forecast, group, threshold and horizon: the four counts of the table pooled over the
    nodes, the pooled scores (the probabilistic ones where the forecast has members) and the FSS per scale; and
    `event_reliability.csv` with one row per forecast with members, group, threshold, horizon and member count j: the forecast
    probability j / K, the number of (window, node) pairs n_j and the observed frequency.  numpy and the standard library
    only.  Returns the three paths."""
    os.makedirs(output_dir, exist_ok=True)
    arrays = {}
    for name, ev in events.items():
        for k in ("count",) + POOLED_COLUMNS + PROB_COLUMNS + ("table",):
            if k not in ev:
                continue
            a = np.asarray(ev[k])
            if grid is not None:
                check_grid(grid, a.shape[-1])
                a = a.reshape(*a.shape[:-1], *[int(d) for d in grid])
            arrays[f"{name}/{k}"] = a
    npz_path = os.path.join(output_dir, "event_maps.npz")
    np.savez_compressed(npz_path, **arrays)
    scales = []
    for ev in events.values():
        scales += [w for w in ev.get("scales", []) if w not in scales]
    csv_path = os.path.join(output_dir, "event_scores.csv")
    with open(csv_path, "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow(["forecast", "group", "threshold", "horizon", "hits", "false_alarms", "misses", "correct_negatives"] +
                    list(POOLED_COLUMNS) + list(PROB_COLUMNS) + [f"fss_{w}" for w in scales] + ["fss_uniform"])
        for name, ev in events.items():
            table = np.asarray(ev["table_pooled"])
            G, Q, H = table.shape[:3]
            for g in range(G):
                for q in range(Q):
                    for h in range(H):
                        row = [name, g, ev["thresholds"][q], h] + [int(v) for v in table[g, q, h]]
                        row += [repr(float(ev[k + "_pooled"][g, q, h])) for k in POOLED_COLUMNS]
                        row += [repr(float(ev[k + "_pooled"][g, q, h])) if k + "_pooled" in ev else "" for k in PROB_COLUMNS]
                        mine = list(ev.get("scales", []))
                        row += [repr(float(ev["fss"][g, q, h, mine.index(w)])) if w in mine else "" for w in scales]
                        row += [repr(float(ev["fss_uniform"][g, q, h])) if "fss_uniform" in ev else ""]
                        wr.writerow(row)
    rel_path = os.path.join(output_dir, "event_reliability.csv")
    with open(rel_path, "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow(["forecast", "group", "threshold", "horizon", "members_yes", "probability", "count", "observed_frequency"])
        for name, ev in events.items():
            if "reliability" not in ev:
                continue
            rel = np.asarray(ev["reliability"])
            G, Q, H, K1 = rel.shape[:4]
            for g in range(G):
                for q in range(Q):
                    for h in range(H):
                        for j in range(K1):
                            wr.writerow([name, g, ev["thresholds"][q], h, j, repr(j / (K1 - 1)), int(rel[g, q, h, j, 0]),
                                         repr(float(rel[g, q, h, j, 1]))])
    return {"npz": npz_path, "csv": csv_path, "reliability": rel_path}
