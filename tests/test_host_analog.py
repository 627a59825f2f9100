"""AnalogBaseline without a GPU: the defaults, what the constructor and the library's host check refuse by name and the
limits they serve, the float64 restatement (tests/analog_ref.py) on a hand-checked 10-row series -- the tie rule, the
exclusion, a key that admits nothing --, the held-out sanity property the GPU test relies on, the names
`tecmollm.evaluate` gives its baselines, and pickling."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import analog_ref as AR
from tests import linear_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tec-mollm_amd", "tecmollm", "libtecmollm_hip.so")


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return LIB


def test_analog_baseline_is_importable_with_its_defaults():
    import tecmollm
    from src.models.baselines import AnalogBaseline, analog_limits
    from tecmollm import evaluate as E
    ab = AnalogBaseline(device="cpu")
    assert ab.k == 16 and ab.match_len is None and ab.channel == 0 and ab.same_slot is True and ab.exclude is None
    assert ab.n_candidates_ is None and ab.match_len_ is None and ab.H_ is None and ab.num_nodes_ is None
    assert E.ANALOG_NAME == "Analog" == tecmollm.ANALOG_NAME and callable(tecmollm.evaluate_analog_ensemble)
    assert "evaluate_analog_ensemble" in tecmollm.__all__ and "analog" in tecmollm.__all__
    assert analog_limits(16, None, 336) == (16, 48)              # the last 48 steps, LinearBaseline's default look-back
    assert analog_limits(16, None, 16) == (16, 16)               # ... or all L_in of them
    assert analog_limits(1, 512, 512, 32) == (1, 512) and analog_limits(32, 1, 4, 1) == (32, 1)


@pytest.mark.parametrize("kw, name", [(dict(k=0), "k must"), (dict(k=33), "k must"), (dict(match_len=0), "match_len"),
                                      (dict(match_len=513), "match_len"), (dict(channel=-1), "channel"),
                                      (dict(exclude=-1), "exclude")])
def test_constructor_refuses_by_name(kw, name):
    from src.models.baselines import AnalogBaseline
    with pytest.raises(ValueError, match=name):
        AnalogBaseline(device="cpu", **kw)
    assert AnalogBaseline(k=32, match_len=512, device="cpu").k == 32          # the limits themselves are served
    assert AnalogBaseline(k=1, match_len=1, exclude=0, device="cpu").match_len == 1


def test_limits_against_the_dataset_are_refused_by_name():
    from src.models.baselines import analog_limits
    for args, name in (((16, 49, 48), "match_len"), ((16, None, 48, 33), "L_out"), ((16, None, 48, 0), "L_out"), ((0, None, 48), "k must")):
        with pytest.raises(ValueError, match=name):
            analog_limits(*args)


def test_host_check_of_the_library_names_what_it_refuses(built_lib):
    from src.models.baselines import analog_search_geometry as geo
    ok = dict(Ta=17520, Ty=17532, Tq=400, N=2911, Cc=6, channel=0, L_in=48, L_out=12, m=48, K=16, S=16)
    chunk, tile, ncand = geo(**ok)
    assert chunk >= 64 and tile >= 1 and ncand == 17520 - 48 + 1 == AR.n_candidates(17520, 17532, 48, 12)
    assert geo(**{**ok, "Ty": 17520})[2] == 17520 - 12 - 48 + 1 == AR.n_candidates(17520, 17520, 48, 12)
    assert geo(**{**ok, "Ta": 40, "Ty": 52})[2] == 0 == AR.n_candidates(40, 52, 48, 12)          # an archive shorter than m: nothing to find
    for change, reason in ((dict(K=0), r"K must lie in \[1, 32\]"), (dict(K=33), r"K must lie in \[1, 32\]"),
                           (dict(m=0), r"m must lie in \[1, 512\]"), (dict(m=513, L_in=600, Tq=700), r"m must lie in \[1, 512\]"),
                           (dict(m=49), "m > L_in"), (dict(L_out=33), r"L_out must lie in \[1, 32\]"), (dict(L_out=0), "L_out must"),
                           (dict(channel=6), "channel"), (dict(channel=-1), "channel"), (dict(Tq=47), "shorter than L_in"),
                           (dict(S=0), "bad shape"), (dict(Ta=1 << 31), "longer than")):
        with pytest.raises(ValueError, match=reason):
            geo(**{**ok, **change})
    # the limits themselves are served
    geo(**{**ok, "K": 32, "m": 512, "L_in": 512, "Tq": 600, "L_out": 32, "Ty": 17552})
    geo(**{**ok, "K": 1, "m": 1, "L_out": 1, "S": 1, "N": 1, "Cc": 1})
    geo(**{**ok, "S": 3000})


# ------------------------------------------------------------------------------------ the restatement, by hand
A10 = np.array([0, 1, 2, 3, 4, 5, 4, 3, 2, 1], dtype=np.float32)[:, None]            # one node
Y10 = 10.0 * A10
SEG = np.array([[[3.0], [3.0]]])                                                     # one query, m = 2


def test_restatement_on_a_ten_row_series_tie_rule_and_mean():
    """m = 2, L_out = 1, Ty = 10: the candidates are c = 0 .. 7 with the segments (0,1) (1,2) (2,3) (3,4) (4,5) (5,4) (4,3) (3,2);
    against (3, 3) their distances are 13 5 1 1 5 5 1 1.  On equal distance the earlier row wins."""
    assert AR.n_candidates(10, 10, 2, 1) == 8
    assert AR.distances(A10, SEG[0], 8)[:, 0].tolist() == [13, 5, 1, 1, 5, 5, 1, 1]
    idx, dist, count = AR.search(A10, 10, SEG, 3, 1)
    assert idx[0, 0].tolist() == [2, 3, 6] and dist[0, 0].tolist() == [1, 1, 1] and count[0, 0] == 3
    idx6, dist6, count6 = AR.search(A10, 10, SEG, 6, 1)
    assert idx6[0, 0].tolist() == [2, 3, 6, 7, 1, 4] and dist6[0, 0].tolist() == [1, 1, 1, 1, 5, 5] and count6[0, 0] == 6
    idx9, dist9, count9 = AR.search(A10, 10, SEG, 9, 1)                                 # fewer candidates than K
    assert idx9[0, 0].tolist() == [2, 3, 6, 7, 1, 4, 5, 0, -1] and count9[0, 0] == 8 and dist9[0, 0, 8] == np.inf
    members, mean = AR.forecast(Y10, idx, count, 2, 1)                                  # the outcomes are Y[c + 2]: 40, 50, 20
    assert members[:, 0, 0, 0].tolist() == [40, 50, 20] and mean[0, 0, 0] == pytest.approx(110 / 3)
    members9, mean9 = AR.forecast(Y10, idx9, count9, 2, 1)
    assert np.isnan(members9[8, 0, 0, 0]) and mean9[0, 0, 0] == pytest.approx((40 + 50 + 20 + 10 + 30 + 40 + 30 + 20) / 8)


def test_restatement_exclusion_keys_and_a_key_that_admits_nothing():
    # the query's origin is row 5; exclude = 2 refuses the origins 4, 5, 6, i.e. c = 2, 3, 4
    idx, dist, count = AR.search(A10, 10, SEG, 3, 1, exclude=2, o_q=[5])
    assert idx[0, 0].tolist() == [6, 7, 1] and dist[0, 0].tolist() == [1, 1, 5] and count[0, 0] == 3
    # keys: the parity of the origin row; key 1 admits the odd origins, i.e. c = 1, 3, 5, 7 with the distances 5 1 5 1
    parity = (np.arange(11) % 2).astype(np.int32)
    idx, dist, count = AR.search(A10, 10, SEG, 3, 1, key_arch=parity, key_q=np.array([1], dtype=np.int32))
    assert idx[0, 0].tolist() == [3, 7, 1] and dist[0, 0].tolist() == [1, 1, 5]
    # both: key 1 and the exclusion leave c = 1, 5, 7
    idx, dist, count = AR.search(A10, 10, SEG, 3, 1, key_arch=parity, key_q=np.array([1], dtype=np.int32), exclude=2, o_q=[5])
    assert idx[0, 0].tolist() == [7, 1, 5] and dist[0, 0].tolist() == [1, 5, 5]
    # a key no archive row carries: nothing is selected and the forecast is NaN
    idx, dist, count = AR.search(A10, 10, SEG, 3, 1, key_arch=parity, key_q=np.array([7], dtype=np.int32))
    assert idx[0, 0].tolist() == [-1, -1, -1] and np.isinf(dist[0, 0]).all() and count[0, 0] == 0
    members, mean = AR.forecast(Y10, idx, count, 2, 1)
    assert np.isnan(members).all() and np.isnan(mean).all()
    # a NaN in the query selects nothing; a NaN in the archive removes the segments that touch it
    idx, _, count = AR.search(A10, 10, np.array([[[np.nan], [3.0]]]), 3, 1)
    assert count[0, 0] == 0 and idx[0, 0].tolist() == [-1, -1, -1]
    dirty = A10.copy()
    dirty[3, 0] = np.nan                                                                # touches c = 2 and c = 3
    idx, _, count = AR.search(dirty, 10, SEG, 3, 1)
    assert idx[0, 0].tolist() == [6, 7, 1] and count[0, 0] == 3


def test_held_out_sanity_property_of_the_restatement():
    """T = 600, m = 48, H = 12, K = 16, seasonal generator, 12 nodes, seed 1, slot = row mod 12; the archive is the record
    behind the first two thirds of the windows, the last third is scored: the analog mean beats the window mean (measured:
    1.018 against 1.208), and every cell finds its 16 analogs."""
    s = AR.held_out_scores(LR.synthetic(600, 12, 1, seasonal=True), np.arange(600) % 12)
    print(s)
    assert s["analog"] < s["mean"] and s["min_count"] == 16


# ------------------------------------------------------------------------------------ names, pickling, refusals before any launch
def test_baseline_name_rules_old_and_new():
    from src.models.baselines import AnalogBaseline, LinearBaseline, SarimaBaseline
    from tecmollm import evaluate as E
    assert [E.baseline_name(k) for k in ("mean", "last", "periodic")] == ["HistoricalAverage", "Persistence", "DayAgo"]
    for bad in ("analog", "Analog", "linear", 3, None):
        with pytest.raises(ValueError, match="baselines must come from"):
            E.baseline_name(bad)
    with pytest.raises(ValueError, match="AnalogBaseline given as a baseline must be fitted"):
        E.baseline_name(AnalogBaseline(device="cpu"))
    with pytest.raises(ValueError, match="LinearBaseline given as a baseline must be fitted"):
        E.baseline_name(LinearBaseline(device="cpu"))
    with pytest.raises(ValueError, match="SarimaBaseline given as a baseline must be fitted"):
        E.baseline_name(SarimaBaseline(device="cpu"))
    ab = AnalogBaseline(device="cpu")
    ab.n_candidates_ = 5
    assert E.baseline_name(ab) == "Analog" == E.ANALOG_NAME
    lb = LinearBaseline(device="cpu")
    lb.coef_ = np.zeros((1, 2, 1))
    assert E.baseline_name(lb) == "Linear"


def test_pickle_holds_numpy_only_and_queries_check_the_fitted_shape():
    from src.models.baselines import AnalogBaseline
    ab = AnalogBaseline(k=3, match_len=2, exclude=4, device="cpu")
    ab.archive_, ab.outcomes_ = np.zeros((3, 10), dtype=np.float32), np.zeros((3, 12), dtype=np.float32)
    ab.slot_ = (np.arange(11) % 12).astype(np.int32)
    ab.n_candidates_, ab.match_len_, ab.H_, ab.num_nodes_, ab.row0_, ab.L_in_ = 9, 2, 2, 3, 0, 4
    ab._A_dev, ab._Y_dev = torch.zeros(3, 10), torch.zeros(3, 12)
    state = ab.__getstate__()
    assert not any(k.startswith("_") for k in state) and not any(isinstance(v, torch.Tensor) for v in state.values())
    assert isinstance(state["device"], str)
    back = pickle.loads(pickle.dumps(ab))
    assert back._A_dev is None and back._Y_dev is None and back._fit_ref is None
    assert np.array_equal(back.archive_, ab.archive_) and np.array_equal(back.slot_, ab.slot_)
    assert back.device == torch.device("cpu") and (back.k, back.match_len_, back.H_, back.exclude) == (3, 2, 2, 4)

    class FakeDataset:
        L_in, L_out, num_samples = 4, 3, 5
        X = torch.zeros(20, 1, 3, 2)
    with pytest.raises(ValueError, match="L_out"):
        back.search_windows(FakeDataset(), [0])
    FakeDataset.L_out, FakeDataset.X = 2, torch.zeros(20, 1, 4, 2)
    with pytest.raises(ValueError, match="num_nodes"):
        back.forecast_windows(FakeDataset(), [0])
    with pytest.raises(ValueError, match="before fit"):
        AnalogBaseline(device="cpu").search_windows(FakeDataset(), [0])
    with pytest.raises(ValueError, match="before fit"):
        AnalogBaseline(device="cpu").predict([0], 1)
    with pytest.raises(ValueError, match="steps"):
        back.predict([0], 3)
