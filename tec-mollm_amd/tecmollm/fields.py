"""Multivariate scores of an ensemble: is a member a plausible TEC *map*?

The per-cell scores (`EnsembleMetrics`: CRPS, spread / skill, coverage, rank histogram) sort the members of every cell, so
members shuffled independently at every node score bit for bit like the coherent ones.  The energy score and the variogram
score (Scheuerer & Hamill 2015) look at whole maps: `FieldMetrics` (src/evaluation/metrics.py) over `tecm_field_scores`.
This module holds what surrounds the kernel: the class matrix that resolves the variogram score by distance
(`pair_classes`, `grid_pair_classes`), the `FieldSpec` that `evaluate_ensemble(..., fields=)` and
`evaluate_analog_ensemble(..., fields=)` take, and the files (`write_fields`).

What it is not: a multivariate rank histogram (its ties need a random tie-break), weights finer than classes, a general
order p, or a score of sub-regions other than through the class matrix (a pair left out of every class is not scored).
"""
from __future__ import annotations

import csv
import os
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np

EXCLUDED = 255          # any value >= the number of classes excludes a pair; this is the one the builders write


def pair_classes(distance_km, edges_km: Sequence[float]) -> np.ndarray:
    """The (I, I) uint8 class matrix of a symmetric (I, I) distance matrix: above the diagonal class c holds the pairs with
    edges[c] < d <= edges[c + 1]; every other pair (d <= edges[0], d > edges[-1], NaN), the diagonal and the lower triangle
    are 255.  `edges_km` are 2 to 17 ascending numbers (the last may be inf): 1 to 16 classes."""
    d = np.asarray(distance_km, dtype=np.float64)
    e = np.asarray(list(edges_km), dtype=np.float64)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError(f"distance_km must be a square matrix, got {d.shape}")
    if e.ndim != 1 or not 2 <= e.size <= 17 or np.isnan(e).any() or not (np.diff(e) > 0).all():
        raise ValueError(f"edges_km must be 2 to 17 strictly ascending numbers, got {list(edges_km)}")
    out = np.full(d.shape, EXCLUDED, dtype=np.uint8)
    for c in range(e.size - 1):
        with np.errstate(invalid="ignore"):
            out[(d > e[c]) & (d <= e[c + 1])] = c
    out[np.tril_indices(d.shape[0])] = EXCLUDED
    return out


def grid_pair_classes(lat, lon, edges_km: Sequence[float]) -> np.ndarray:
    """`pair_classes` of the Haversine distances of the regular lat / lon grid (node = lat index * n_lon + lon index, as
    `src.graph.graph_constructor` numbers them).  Dense: 8.5 MB of classes and a float64 distance matrix at N = 2911."""
    from src.graph.graph_constructor import calculate_haversine_distance_matrix
    return pair_classes(calculate_haversine_distance_matrix(np.asarray(lat), np.asarray(lon)), edges_km)


@dataclass
class FieldSpec:
    """What `evaluate_ensemble(..., fields=)` needs for the field scores: the (N, N) uint8 class matrix (numpy or torch; None
    for the energy score alone), the class edges it was built from (labels of the files; None numbers the classes) and the
    order of the variogram score (0.5, 1 or 2)."""
    pair_class: Optional[object] = None
    edges_km: Optional[Sequence[float]] = None
    order: float = 0.5

    @property
    def num_classes(self) -> int:
        if self.pair_class is None:
            return 0
        if self.edges_km is not None:
            return len(list(self.edges_km)) - 1
        import torch
        pc = torch.as_tensor(self.pair_class)
        live = pc[pc != EXCLUDED]
        return int(live.max()) + 1 if live.numel() else 1

    def metrics(self, num_horizons: int, num_nodes: int, members: int, num_groups: int, scaler, device):
        """The `FieldMetrics` of this specification."""
        import torch
        from src.evaluation.metrics import FieldMetrics
        pc = None if self.pair_class is None else torch.as_tensor(self.pair_class)
        return FieldMetrics(num_horizons, num_nodes, members, pc, self.num_classes, self.order, num_groups, scaler, device=device)

    def entries(self, computed: Dict[str, object]) -> Dict[str, object]:
        """What `evaluate_ensemble` adds to `prob`: `FieldMetrics.compute()` with its sample count under "field_count" (G, H)
        -- `prob["count"]` is, and stays, the per-cell count (G, H, N) of `EnsembleMetrics` -- plus `describe()`."""
        out = {("field_count" if k == "count" else k): v for k, v in computed.items()}
        out.update(self.describe())
        return out

    def describe(self) -> Dict[str, object]:
        """The entries that go into `prob` next to the scores, so that `write_fields` can label its rows."""
        edges = None if self.edges_km is None else [float(v) for v in self.edges_km]
        return {"field_order": float(self.order), "field_edges_km": edges}


CSV_COLUMNS = ("count", "pairs", "variogram_score", "variogram_score_per_pair", "variogram_obs", "variogram_ens",
               "variogram_ratio", "energy_score", "fair_energy_score", "field_error_mean")


def write_fields(prob: Dict[str, object], output_dir: str) -> Dict[str, str]:
    """The files of the field scores in `prob` (`FieldMetrics.compute()`, or the third result of `evaluate_ensemble(...,
    fields=)`, where the sample count is "field_count"): `field_scores.npz` with one array per key of `FIELD_KEYS` plus
    `order` and `edges_km` where known; and
    `field_scores.csv` with, per group and horizon, one row per class (the variogram columns) and one row "energy" (the
    energy columns); the columns that do not apply to a row stay empty.  numpy and the standard library only.  Returns the
    two paths."""
    from src.evaluation.metrics import FIELD_KEYS
    os.makedirs(output_dir, exist_ok=True)
    arrays = {k: np.asarray(prob["field_count"] if k == "count" and "field_count" in prob else prob[k]) for k in FIELD_KEYS}
    edges = prob.get("field_edges_km")
    if prob.get("field_order") is not None:
        arrays["order"] = np.asarray(float(prob["field_order"]))
    if edges is not None:
        arrays["edges_km"] = np.asarray(edges, dtype=np.float64)
    npz_path = os.path.join(output_dir, "field_scores.npz")
    np.savez_compressed(npz_path, **arrays)
    G, H, NB = arrays["variogram_score"].shape
    vario = CSV_COLUMNS[1:7]
    csv_path = os.path.join(output_dir, "field_scores.csv")
    with open(csv_path, "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow(["group", "horizon", "class", "lo_km", "hi_km"] + list(CSV_COLUMNS))
        for g in range(G):
            for h in range(H):
                n = repr(float(arrays["count"][g, h]))
                for c in range(NB):
                    lo, hi = (repr(float(edges[c])), repr(float(edges[c + 1]))) if edges is not None else ("", "")
                    wr.writerow([g, h, c, lo, hi, n] + [repr(float(arrays[k][g, h, c])) for k in vario] + ["", "", ""])
                wr.writerow([g, h, "energy", "", "", n] + [""] * len(vario)
                            + [repr(float(arrays[k][g, h])) for k in CSV_COLUMNS[7:]])
    return {"npz": npz_path, "csv": csv_path}
