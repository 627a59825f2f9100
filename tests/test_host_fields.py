"""Host tests of the field scores: the class matrix (`pair_classes`), `derive_fields` against hand-computed cases, the
library's plan function and what it refuses, the files, and the restatement (tests/fields_ref.py) on the property that
motivates the feature: members shuffled independently at every node keep every per-cell CRPS sum bit for bit and at least
double the short-range variogram score."""
import os
import re

import numpy as np
import pytest

from tests import ensemble_ref as ER
from tests import fields_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tec-mollm_amd", "tecmollm", "libtecmollm_hip.so")
SCALER = (21.5, 9.25)


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return LIB


def test_pair_classes_edges_diagonal_lower_triangle_and_nan():
    from tecmollm.fields import EXCLUDED, pair_classes
    d = np.array([[0.0, 150.0, 150.0000001, 700.0],
                  [150.0, 0.0, np.nan, 300.0],
                  [150.0000001, np.nan, 0.0, 0.0],
                  [700.0, 300.0, 0.0, 0.0]])
    pc = pair_classes(d, (0.0, 150.0, 300.0, 600.0))
    assert pc.dtype == np.uint8 and pc.shape == (4, 4) and EXCLUDED == 255
    want = np.full((4, 4), 255, dtype=np.uint8)
    want[0, 1] = 0            # d == 150: edges[0] < d <= edges[1]
    want[0, 2] = 1            # just above 150
    want[1, 3] = 1            # d == 300 closes class 1
    # (0, 3): 700 > the last edge; (1, 2): NaN; (2, 3): 0 is not > edges[0]; diagonal and lower triangle: 255
    assert np.array_equal(pc, want)
    open_end = pair_classes(d, (0.0, 150.0, np.inf))
    assert open_end[0, 3] == 1 and open_end[1, 2] == 255 and (np.tril(open_end) == np.tril(np.full((4, 4), 255))).all()
    for bad in ((0.0,), (0.0, 0.0), (1.0, 0.5), (0.0, np.nan), tuple(range(18))):
        with pytest.raises(ValueError):
            pair_classes(d, bad)
    with pytest.raises(ValueError):
        pair_classes(d[:3], (0.0, 1.0))


def test_grid_pair_classes_uses_the_graph_builders_distances():
    from src.graph.graph_constructor import calculate_haversine_distance_matrix
    from tecmollm.fields import grid_pair_classes, pair_classes
    lat, lon = 30.0 + np.arange(3), 100.0 + np.arange(4)
    pc = grid_pair_classes(lat, lon, (0, 150, 300, np.inf))
    assert np.array_equal(pc, pair_classes(calculate_haversine_distance_matrix(lat, lon), (0, 150, 300, np.inf)))
    assert pc[0, 1] == 0 and pc[0, 4] == 0 and pc[0, 3] == 1 and pc[0, 11] == 2     # neighbours ~96 / 111 km, three columns ~289 km
    np.testing.assert_allclose(FR.grid_distances(3, 4), calculate_haversine_distance_matrix(lat, lon), rtol=1e-12)


def test_derive_fields_on_hand_computed_cases():
    from src.evaluation.metrics import FIELD_KEYS, derive_fields
    # K = 2, two windows: A sums to 6, D to 4, E to 3;  one class: 10 pairs, sum e^2 = 5, sum v_o = 20, sum v_e = 15
    es = np.array([[2.0, 6.0, 4.0, 3.0], [0.0, 0.0, 0.0, 0.0]])
    vs = np.array([[[2.0, 10.0, 5.0, 20.0, 15.0], [2.0, 0.0, 0.0, 0.0, 0.0]], [[0.0] * 5, [0.0] * 5]])
    out = derive_fields(es, vs, 2)
    assert set(out) == set(FIELD_KEYS)
    assert out["count"].tolist() == [2.0, 0.0] and out["pairs"].tolist() == [[10.0, 0.0], [0.0, 0.0]]
    assert out["energy_score"][0] == 3.0 - 2.0 / 4 and out["fair_energy_score"][0] == 3.0 - 2.0 / 2 and out["field_error_mean"][0] == 1.5
    assert out["variogram_score"][0, 0] == 2.5 and out["variogram_score_per_pair"][0, 0] == 0.5
    assert out["variogram_obs"][0, 0] == 2.0 and out["variogram_ens"][0, 0] == 1.5 and out["variogram_ratio"][0, 0] == 0.75
    assert out["variogram_score"][0, 1] == 0.0                      # seen, but the class is empty: the score is 0 ...
    for k in ("variogram_score_per_pair", "variogram_obs", "variogram_ens", "variogram_ratio"):
        assert np.isnan(out[k][0, 1])                               # ... and what is per pair is NaN
    for k in FIELD_KEYS[1:4] + FIELD_KEYS[5:]:
        assert np.isnan(out[k][1]).all(), k                         # nothing seen: NaN
    nb0 = derive_fields(es, np.zeros((2, 0, 5)), 2)
    assert nb0["variogram_score"].shape == (2, 0) and nb0["energy_score"][0] == 2.5
    with pytest.raises(ValueError):
        derive_fields(es, vs[:1], 2)
    with pytest.raises(ValueError):
        derive_fields(es[:, :3], vs, 2)


def test_one_member_has_no_fair_score_and_its_energy_score_is_the_field_error():
    from src.evaluation.metrics import derive_fields
    rng = np.random.default_rng(3)
    m = rng.standard_normal((1, 4, 2, 9)).astype(np.float32)
    t = rng.standard_normal((4, 2, 9)).astype(np.float32)
    es, mags = np.zeros((1, 2, 4)), np.zeros((1, 2, 4))
    q = FR.accumulate(es, mags, np.zeros((1, 2, 0, 5)), np.zeros((1, 2, 0, 3)), m, t, None, SCALER)
    assert np.array_equal(q["es"][..., 1], np.zeros((4, 2)))        # no pair of members
    assert np.array_equal(q["es"][..., 0], q["es"][..., 2])         # A of the one member is E, bit for bit
    out = derive_fields(es, np.zeros((1, 2, 0, 5)), 1)
    assert np.isnan(out["fair_energy_score"]).all()
    assert np.array_equal(out["energy_score"], out["field_error_mean"]) and (out["energy_score"] > 0).all()


def test_the_plan_function_answers_and_names_what_it_refuses(built_lib):
    from tecmollm import _lib, ops
    T, lds, ws = ops.field_scores_plan(16, 12, 2911, 16, 8)
    nt = -(-2911 // T)
    assert T in (64, 128) and lds <= 160 * 1024 and lds >= 17 * 2 * T * 4
    assert ws >= 8 * 16 * 12 * (nt * (nt + 1) // 2) * 8 * 4         # at least the pair partials
    assert ops.field_scores_plan(16, 12, 2911, 64, 16)[1] <= 160 * 1024          # the largest K and NB still fit
    T0, lds0, ws0 = ops.field_scores_plan(5, 1, 7, 1, 0)                          # the energy score alone
    assert T0 in (64, 128) and 0 < lds0 <= 64 * 1024 and 0 < ws0 < ws
    for change, reason in ((dict(K=0), r"K = 0 outside \[1, 64\]"), (dict(K=65), r"K = 65 outside \[1, 64\]"),
                           (dict(NB=17), r"NB = 17 outside \[0, 16\]"), (dict(NB=-1), r"NB = -1 outside"),
                           (dict(S=0), "bad shape"), (dict(I=0), "bad shape"), (dict(H=0), "bad shape"),
                           (dict(S=65536), "S and H must be <= 65535"), (dict(H=65536), "S and H must be <= 65535"),
                           (dict(I=128 * 65535 + 1, NB=0), "more than 65535 tiles")):
        args = {**dict(S=16, H=12, I=2911, K=16, NB=8), **change}
        with pytest.raises(_lib.TecmError, match=reason):
            ops.field_scores_plan(**args)
    header = open(os.path.join(ROOT, "include", "tecmollm.h")).read()
    assert _lib.ABI_VERSION == 21 == int(re.search(r"#define\s+TECM_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.lib().tecm_abi_version()
    assert f"#define TECM_FIELD_MAX_CLASSES {_lib.TECM_FIELD_MAX_CLASSES}" in header
    assert f"#define TECM_FIELD_ES_STATS {_lib.TECM_FIELD_ES_STATS}" in header and f"#define TECM_FIELD_VS_STATS {_lib.TECM_FIELD_VS_STATS}" in header
    assert "TECM_FIELD_ORDER_HALF = 0, TECM_FIELD_ORDER_ONE = 1, TECM_FIELD_ORDER_TWO = 2" in header
    assert ops.FIELD_ORDERS == {0.5: 0, 1.0: 1, 2.0: 2}


def test_the_build_lists_the_kernels_with_a_scratch_ceiling_of_zero():
    import __graft_entry__ as g
    from tecmollm import _lib
    assert "field_scores.hip" in g.SOURCES
    rules = g.SPILL_CEILINGS["field_scores.hip"]
    assert {r[0] for r in rules} == {f"field_{k}_kernel" for k in ("pairs", "pairs_sample", "energy", "energy_sample", "cells")}
    assert all(r[1] == "ScratchSize [bytes/lane]" and r[2] == 0 for r in rules)
    assert {"tecm_field_scores", "tecm_field_scores_plan"} <= set(_lib.EXPORTS)


def test_the_restatement_sees_the_shuffle_that_the_per_cell_scores_cannot():
    """9 x 13 one-degree grid, exponential covariance with a 500 km range, K = 8, S = 6, H = 3, classes at 150 / 300 / 600 km,
    order 0.5, seed 0: the per-cell sums behind the CRPS are identical, the pooled first-class variogram score at least
    doubles, every class gets worse with the effect fading with distance, and the energy score rises a little."""
    from tecmollm.fields import pair_classes
    members, shuffled, truth, d = FR.coherent_and_shuffled(0)
    assert members.shape == (8, 6, 3, 117) and not np.array_equal(members, shuffled)
    assert np.array_equal(np.sort(members, axis=0), np.sort(shuffled, axis=0))
    a, b = ER.per_sample(members, truth, SCALER, 0), ER.per_sample(shuffled, truth, SCALER, 0)
    for k in ("A", "D", "mu", "var", "rank", "width"):
        assert np.array_equal(a[k], b[k]), k
    pc = pair_classes(d, (0.0, 150.0, 300.0, 600.0, np.inf))
    qa = FR.per_sample(members, truth, SCALER, pc, 4, 0.5)
    qb = FR.per_sample(shuffled, truth, SCALER, pc, 4, 0.5)
    assert np.array_equal(qa["vs"][..., 0], qb["vs"][..., 0]) and qa["vs"][0, 0, :, 0].sum() == 117 * 116 // 2
    ratio = qb["vs"][..., 1].sum(axis=(0, 1)) / qa["vs"][..., 1].sum(axis=(0, 1))
    print("pooled shuffled / coherent variogram score by class:", ratio)
    assert ratio[0] >= 2.0 and (ratio > 1.0).all() and (np.diff(ratio) < 0).all()
    assert np.array_equal(qa["vs"][..., 2], qb["vs"][..., 2])       # the observed variogram does not know the members
    es = [(q["es"][..., 0] - q["es"][..., 1] / 64).mean() for q in (qa, qb)]
    assert 1.005 < es[1] / es[0] < 1.1
    assert np.array_equal(qa["es"][..., 2], qb["es"][..., 2])       # the ensemble-mean map is the same


def test_field_spec_and_the_files_round_trip(tmp_path):
    from src.evaluation.metrics import FIELD_KEYS, derive_fields
    from tecmollm.fields import CSV_COLUMNS, FieldSpec, pair_classes, write_fields
    d = FR.grid_distances(2, 3)
    edges = (0.0, 150.0, 300.0)
    spec = FieldSpec(pair_classes(d, edges), edges, 1.0)
    assert spec.num_classes == 2 and spec.describe() == {"field_order": 1.0, "field_edges_km": [0.0, 150.0, 300.0]}
    assert FieldSpec().num_classes == 0 and FieldSpec(pair_classes(d, edges)).num_classes == 2
    rng = np.random.default_rng(1)
    es, vs = rng.random((2, 3, 4)) + 1.0, rng.random((2, 3, 2, 5)) + 1.0
    es[1, 2] = 0.0
    vs[1, 2] = 0.0
    prob = dict(derive_fields(es, vs, 4), crps=np.zeros(3), **spec.describe())
    paths = write_fields(prob, str(tmp_path / "out"))
    z = np.load(paths["npz"])
    assert sorted(z.files) == sorted(FIELD_KEYS + ("order", "edges_km"))
    for k in FIELD_KEYS:
        assert np.array_equal(z[k], prob[k], equal_nan=True), k
    assert float(z["order"]) == 1.0 and z["edges_km"].tolist() == list(edges)
    with open(paths["csv"], encoding="utf-8") as f:
        lines = [ln.split(",") for ln in f.read().splitlines()]
    assert lines[0] == ["group", "horizon", "class", "lo_km", "hi_km"] + list(CSV_COLUMNS) and len(lines) == 1 + 2 * 3 * 3
    row = lines[1 + (0 * 3 + 1) * 3 + 1]                               # group 0, horizon 1, class 1
    assert row[:5] == ["0", "1", "1", "150.0", "300.0"] and float(row[5 + 2]) == prob["variogram_score"][0, 1, 1] and row[-1] == ""
    erow = lines[1 + (0 * 3 + 1) * 3 + 2]
    assert erow[2] == "energy" and float(erow[-3]) == prob["energy_score"][0, 1] and erow[6] == ""
    assert lines[-1][-1] == "nan"                                      # the cell that saw nothing
    bare = write_fields(derive_fields(es, vs, 4), str(tmp_path / "bare"))
    assert sorted(np.load(bare["npz"]).files) == sorted(FIELD_KEYS)
    # next to the per-cell scores of an ensemble the sample count goes by "field_count": "count" stays the per-cell one
    merged = {"count": np.zeros((2, 3, 6)), "crps": np.zeros((2, 3, 6))}
    merged.update(spec.entries(derive_fields(es, vs, 4)))
    assert merged["count"].shape == (2, 3, 6) and np.array_equal(merged["field_count"], es[..., 0])
    assert set(merged) == {"crps", "field_count", "field_order", "field_edges_km"} | set(FIELD_KEYS)
    again = np.load(write_fields(merged, str(tmp_path / "merged"))["npz"])
    assert all(np.array_equal(again[k], z[k], equal_nan=True) for k in z.files)
