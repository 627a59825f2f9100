"""tecmollm -- MI355X (gfx950) implementation of the TEC-MoLLM forward/backward hot path.

Package layout (inside `tec-mollm_amd/`, which must be on sys.path):
  csrc/            hand-written HIP kernels + the C ABI (include/tecmollm.h at the repo root)
  tecmollm/        ctypes binding, autograd stage functions, graph preparation, training-step helpers, test-split evaluation,
                   input attribution, ensemble forecasts and their scores, spatial and temporal attention maps, conformal
                   prediction intervals, significance of the comparison (block bootstrap, Diebold-Mariano), event verification
                   (contingency scores, Brier, ROC, FSS), quantile forecasts (pinball-loss training, quantile scores,
                   conformalized quantile regression), forecast combination (per-cell stacking weights), the analog ensemble's
                   probabilistic scores, multivariate ensemble scores (energy and variogram score), coherent ensemble maps (ECC and
                   Schaake-shuffle reordering), raw-data preprocessing
  src/model/       mirror of the reference's module API (`from src.model.tec_mollm import TEC_MoLLM`)
  src/features/    mirror of the reference's feature engineering (`from src.features.feature_engineering import ...`)
  src/data/        mirrors of the reference's dataset and data loader, and the series-backed SeriesWindowDataset
  src/models/      mirror of the reference's baselines (`from src.models.baselines import HistoricalAverage`)
"""
from ._lib import LIB_PATH, TecmError, lib  # noqa: F401
from .devcheck import check_device_errors  # noqa: F401
from .attribute import attribution_maps, input_gradient, integrated_gradients, write_attributions  # noqa: F401
from .functions import PinballFn, PinballLoss, dropout_seed  # noqa: F401
from . import ensemble  # noqa: F401
from .ensemble import (ensemble_forecast, ensemble_members, evaluate_ensemble, member_seed,  # noqa: F401
                       write_ensemble)
from . import conformal  # noqa: F401
from .conformal import (ConformalCalibrator, ConformalIntervals, calibrate_conformal, conformal_forecast,  # noqa: F401
                        conformal_ranks, evaluate_conformal, write_conformal)
from .spatial_attention import (AttentionStats, attention_maps, evaluate_attention, graph_groups_by_lag,  # noqa: F401
                                graph_groups_by_sample, graph_groups_by_slot, spatial_attention, write_attention)
from .temporal_attention import (TemporalAttentionStats, evaluate_temporal_attention, temporal_attention,  # noqa: F401
                                 write_temporal_attention)
from . import significance  # noqa: F401
from .significance import (WindowScores, block_bootstrap, bootstrap_intervals, diebold_mariano,  # noqa: F401
                           evaluate_significance, score_windows, write_significance)
from . import events  # noqa: F401
from .events import EventThresholds, evaluate_events, target_slots, write_events  # noqa: F401
from . import quantile  # noqa: F401
from .quantile import (CQRIntervals, QuantileModel, calibrate_cqr, evaluate_quantiles, quantile_config,  # noqa: F401
                       quantile_forecast, write_quantiles)
from . import combine  # noqa: F401
from .combine import Combination, CombinationMoments, fit_combination, write_combination  # noqa: F401
from . import analog  # noqa: F401
from .analog import evaluate_analog_ensemble  # noqa: F401
from .evaluate import ANALOG_NAME  # noqa: F401
from . import fields  # noqa: F401
from .fields import FieldSpec, grid_pair_classes, pair_classes, write_fields  # noqa: F401
from . import coherence  # noqa: F401
from .coherence import (EccTemplate, SchaakeTemplate, evaluate_quantile_ensemble, quantile_members,  # noqa: F401
                        reorder_members)
from . import preprocess  # noqa: F401
from .preprocess import DeviceStandardScaler, preprocess_splits  # noqa: F401

__all__ = ["LIB_PATH", "TecmError", "lib", "check_device_errors", "input_gradient", "integrated_gradients",
           "attribution_maps", "write_attributions", "dropout_seed", "ensemble", "member_seed", "ensemble_members",
           "ensemble_forecast", "evaluate_ensemble", "write_ensemble", "spatial_attention", "AttentionStats",
           "evaluate_attention", "attention_maps", "write_attention", "graph_groups_by_sample", "graph_groups_by_slot",
           "graph_groups_by_lag", "conformal", "conformal_ranks", "ConformalCalibrator", "ConformalIntervals",
           "calibrate_conformal", "conformal_forecast", "evaluate_conformal", "write_conformal", "temporal_attention",
           "TemporalAttentionStats", "evaluate_temporal_attention", "write_temporal_attention", "preprocess", "DeviceStandardScaler",
           "preprocess_splits", "significance", "WindowScores", "score_windows", "block_bootstrap", "bootstrap_intervals",
           "diebold_mariano", "evaluate_significance", "write_significance", "events", "EventThresholds", "target_slots",
           "evaluate_events", "write_events", "quantile", "PinballFn", "PinballLoss", "QuantileModel", "CQRIntervals",
           "quantile_config", "quantile_forecast", "evaluate_quantiles", "calibrate_cqr", "write_quantiles", "combine", "Combination",
           "CombinationMoments", "fit_combination", "write_combination", "analog", "evaluate_analog_ensemble",
           "ANALOG_NAME", "fields", "FieldSpec", "pair_classes", "grid_pair_classes", "write_fields",
           "coherence", "reorder_members", "SchaakeTemplate", "EccTemplate", "quantile_members", "evaluate_quantile_ensemble"]
