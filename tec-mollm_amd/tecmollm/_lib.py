"""ctypes binding of libtecmollm_hip.so (C ABI: include/tecmollm.h).

The product path has no CPU fallback: if the HIP library is missing, `lib()` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TECM_LIB", os.path.join(_HERE, "libtecmollm_hip.so"))   # override for experiments
ABI_VERSION = 21

c_f32p = C.c_void_p


class TecmWin(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("N", C.c_int32), ("Lin", C.c_int32), ("Lout", C.c_int32),
                ("stride_t", C.c_int32), ("taps", C.c_int32), ("Cw", C.c_int32), ("pad", C.c_int32)]


class TecmDrop(C.Structure):
    _fields_ = [("p", C.c_float), ("_pad", C.c_int32), ("seed", C.c_uint64), ("ld", C.c_int64), ("seed_dev", C.c_void_p)]


class TecmGemm(C.Structure):
    _fields_ = [
        ("M", C.c_int64), ("N", C.c_int64), ("K", C.c_int64),
        ("A", c_f32p), ("lda", C.c_int64), ("a_layout", C.c_int32), ("io_bf16", C.c_int32),
        ("a_win", TecmWin), ("a_drop", TecmDrop),
        ("B", c_f32p), ("ldb", C.c_int64), ("b_layout", C.c_int32), ("_p1", C.c_int32),
        ("b_win", TecmWin), ("b_drop", TecmDrop),
        ("C", c_f32p), ("ldc", C.c_int64), ("c_win", TecmWin),
        ("alpha", C.c_float), ("act", C.c_int32),
        ("bias", c_f32p),
        ("rowbias", c_f32p), ("rb_ld", C.c_int64), ("rb_div", C.c_int32), ("rb_mod", C.c_int32),
        ("preact", c_f32p), ("ldp", C.c_int64),
        ("dact_src", c_f32p), ("ldd", C.c_int64),
        ("out_drop", TecmDrop),
        ("residual", c_f32p), ("ldr", C.c_int64),
        ("accumulate", C.c_int32), ("split_k", C.c_int32),
        ("workspace", c_f32p),
        ("dead_period", C.c_int32), ("dead_rows", C.c_int32), ("dead_cols", C.c_int32),
        ("zero_period", C.c_int32), ("zero_rows", C.c_int32), ("zero_k", C.c_int32),
    ]


class TecmSpatial(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("L", C.c_int32), ("N", C.c_int32), ("Cin", C.c_int32), ("Demb", C.c_int32),
        ("H", C.c_int32), ("graphs_with_edges", C.c_int32),
        ("num_tiles", C.c_int32), ("tile_nodes", C.c_int32), ("win_max", C.c_int32),
        ("x", c_f32p),
        ("tf", c_f32p), ("tf_sb", C.c_int64), ("tf_sl", C.c_int64), ("tf_sn", C.c_int64), ("tf_sf", C.c_int64),
        ("node_tab", c_f32p), ("tod_tab", c_f32p), ("doy_tab", c_f32p), ("year_tab", c_f32p),
        ("season_tab", c_f32p),
        ("year_rows", C.c_int32), ("tile_edges_max", C.c_int32),
        ("Wl", c_f32p), ("bl", c_f32p), ("Wr", c_f32p), ("br", c_f32p),
        ("att", c_f32p), ("bias", c_f32p),
        ("rowptr", C.c_void_p), ("colidx", C.c_void_p), ("tile_lo", C.c_void_p), ("tile_hi", C.c_void_p),
        ("alpha_drop", TecmDrop),
        ("out", c_f32p),
        ("err_flag", C.c_void_p),
        ("flags", C.c_int32), ("out_ld", C.c_int32),
    ]


class TecmSpatialGrads(C.Structure):
    _fields_ = [
        ("dout", c_f32p), ("d_node_tab", c_f32p), ("d_tod_tab", c_f32p), ("d_doy_tab", c_f32p),
        ("d_year_tab", c_f32p), ("d_season_tab", c_f32p),
        ("partials", c_f32p), ("partial_ld", C.c_int64),
        ("t_chunk", C.c_int32), ("num_blocks", C.c_int32),
        ("src_ptr", C.c_void_p), ("src_col", C.c_void_p), ("src_ptr_off", C.c_void_p),
    ]


class TecmSpatialDx(C.Structure):
    _fields_ = [
        ("dout", c_f32p), ("dx", c_f32p), ("dx_ld", C.c_int64), ("ws", c_f32p),
        ("src_rowptr", C.c_void_p), ("src_target", C.c_void_p), ("src_slot", C.c_void_p),
    ]


class TecmSpatialAttn(C.Structure):
    _fields_ = [
        ("alpha", c_f32p), ("perm", C.c_void_p), ("edge_stats", C.c_void_p), ("node_stats", C.c_void_p),
        ("counts", C.c_void_p), ("group", C.c_void_p), ("ws", c_f32p), ("ws_floats", C.c_int64),
        ("num_groups", C.c_int32), ("E", C.c_int32), ("flags", C.c_int32), ("_pad", C.c_int32),
    ]


class TecmTemporalAttn(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("probs", c_f32p), ("nodes", C.c_void_p), ("node_stats", C.c_void_p),
        ("lag_stats", C.c_void_p), ("matrix_stats", C.c_void_p), ("counts", C.c_void_p), ("group", C.c_void_p),
        ("err_flag", C.c_void_p), ("ws", c_f32p), ("ws_floats", C.c_int64),
        ("B", C.c_int32), ("T", C.c_int32), ("N", C.c_int32), ("heads", C.c_int32), ("D", C.c_int32), ("Ns", C.c_int32),
        ("num_groups", C.c_int32), ("num_layers", C.c_int32), ("layer", C.c_int32), ("flags", C.c_int32),
    ]


class TecmLnAdd(C.Structure):
    _fields_ = [("dy2", C.c_void_p), ("ld", C.c_int64), ("bf16", C.c_int32), ("_pad", C.c_int32), ("drop", TecmDrop)]


class TecmLnDyMap(C.Structure):
    _fields_ = [("T", C.c_int32), ("N", C.c_int32), ("drop", TecmDrop)]


class TecmAdamW(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("param", c_f32p), ("grad", c_f32p), ("exp_avg", c_f32p), ("exp_avg_sq", c_f32p),
        ("partials", C.c_void_p), ("total_norm_out", c_f32p),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("weight_decay", C.c_float), ("max_norm", C.c_float), ("grad_scale", C.c_float),
        ("step", C.c_int32), ("zero_grad", C.c_int32), ("_pad", C.c_int32),
    ]


class TecmMetrics(C.Structure):
    _fields_ = [
        ("pred", c_f32p), ("p_stride_s", C.c_int64), ("p_stride_h", C.c_int64), ("p_stride_i", C.c_int64),
        ("target", c_f32p), ("t_stride_s", C.c_int64), ("t_stride_h", C.c_int64), ("t_stride_i", C.c_int64),
        ("S", C.c_int64), ("H", C.c_int32), ("_pad", C.c_int32), ("I", C.c_int64),
        ("mean", C.c_double), ("scale", C.c_double),
        ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("clip", C.c_int32), ("_pad2", C.c_int32),
        ("stats", C.c_void_p),
    ]


class TecmMetricsMap(C.Structure):
    _fields_ = [
        ("pred", c_f32p), ("p_stride_s", C.c_int64), ("p_stride_h", C.c_int64), ("p_stride_i", C.c_int64),
        ("target", c_f32p), ("t_stride_s", C.c_int64), ("t_stride_h", C.c_int64), ("t_stride_i", C.c_int64),
        ("S", C.c_int64), ("H", C.c_int32), ("G", C.c_int32), ("I", C.c_int64),
        ("mean", C.c_double), ("scale", C.c_double),
        ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("clip", C.c_int32), ("_pad2", C.c_int32),
        ("stats", C.c_void_p), ("group", C.c_void_p), ("err_flag", C.c_void_p),
    ]


class TecmEnsemble(C.Structure):
    _fields_ = [
        ("members", c_f32p), ("m_stride_k", C.c_int64), ("m_stride_s", C.c_int64), ("m_stride_h", C.c_int64),
        ("m_stride_i", C.c_int64),
        ("target", c_f32p), ("t_stride_s", C.c_int64), ("t_stride_h", C.c_int64), ("t_stride_i", C.c_int64),
        ("S", C.c_int64), ("H", C.c_int32), ("G", C.c_int32), ("I", C.c_int64),
        ("K", C.c_int32), ("trim", C.c_int32),
        ("mean", C.c_double), ("scale", C.c_double),
        ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("clip", C.c_int32), ("_pad2", C.c_int32),
        ("stats", C.c_void_p), ("hist", C.c_void_p), ("group", C.c_void_p), ("err_flag", C.c_void_p),
        ("out_mean", c_f32p), ("out_std", c_f32p), ("out_lo", c_f32p), ("out_hi", c_f32p), ("out_mean_raw", c_f32p),
        ("o_stride_s", C.c_int64), ("o_stride_h", C.c_int64), ("o_stride_i", C.c_int64),
    ]


class TecmConformalScores(C.Structure):
    _fields_ = [
        ("pred", c_f32p), ("p_stride_s", C.c_int64), ("p_stride_h", C.c_int64), ("p_stride_i", C.c_int64),
        ("target", c_f32p), ("t_stride_s", C.c_int64), ("t_stride_h", C.c_int64), ("t_stride_i", C.c_int64),
        ("sigma", c_f32p), ("g_stride_s", C.c_int64), ("g_stride_h", C.c_int64), ("g_stride_i", C.c_int64),
        ("S", C.c_int64), ("H", C.c_int32), ("mode", C.c_int32), ("I", C.c_int64),
        ("mean", C.c_double), ("scale", C.c_double),
        ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("clip", C.c_int32), ("sigma_min", C.c_float),
        ("scores", c_f32p), ("ld", C.c_int64), ("row0", C.c_int64),
    ]


class TecmColumnSelect(C.Structure):
    _fields_ = [
        ("x", c_f32p), ("ld", C.c_int64), ("S", C.c_int64), ("C", C.c_int64),
        ("group", C.c_void_p), ("ranks", C.c_void_p), ("G", C.c_int32), ("Q", C.c_int32),
        ("out", c_f32p), ("err_flag", C.c_void_p),
    ]


class TecmIntervalStats(C.Structure):
    _fields_ = [
        ("pred", c_f32p), ("p_stride_s", C.c_int64), ("p_stride_h", C.c_int64), ("p_stride_i", C.c_int64),
        ("target", c_f32p), ("t_stride_s", C.c_int64), ("t_stride_h", C.c_int64), ("t_stride_i", C.c_int64),
        ("sigma", c_f32p), ("g_stride_s", C.c_int64), ("g_stride_h", C.c_int64), ("g_stride_i", C.c_int64),
        ("S", C.c_int64), ("H", C.c_int32), ("mode", C.c_int32), ("I", C.c_int64),
        ("mean", C.c_double), ("scale", C.c_double),
        ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("clip", C.c_int32), ("sigma_min", C.c_float),
        ("q_lo", c_f32p), ("q_hi", c_f32p), ("Gq", C.c_int32), ("G", C.c_int32),
        ("alpha", C.c_double),
        ("stats", C.c_void_p), ("group", C.c_void_p), ("err_flag", C.c_void_p),
        ("out_lo", c_f32p), ("out_hi", c_f32p), ("out_mid", c_f32p),
        ("o_stride_s", C.c_int64), ("o_stride_h", C.c_int64), ("o_stride_i", C.c_int64),
    ]


TECM_QUANT_MAX_Q = 16
TECM_PINBALL_BLOCK_CAP = 1024


class TecmPinball(C.Structure):
    _fields_ = [
        ("pred", c_f32p), ("p_stride_b", C.c_int64), ("p_stride_q", C.c_int64), ("p_stride_h", C.c_int64),
        ("p_stride_n", C.c_int64),
        ("target", c_f32p), ("t_stride_b", C.c_int64), ("t_stride_h", C.c_int64), ("t_stride_n", C.c_int64),
        ("B", C.c_int32), ("Q", C.c_int32), ("H", C.c_int32), ("N", C.c_int32),
        ("taus", C.c_float * TECM_QUANT_MAX_Q),
        ("grad_scale", C.c_float), ("_pad", C.c_int32),
        ("dpred", c_f32p), ("loss_out", c_f32p), ("loss_levels", c_f32p), ("workspace", C.c_void_p),
    ]


class TecmQuantileStats(C.Structure):
    _fields_ = [
        ("levels", c_f32p), ("l_stride_q", C.c_int64), ("l_stride_s", C.c_int64), ("l_stride_h", C.c_int64),
        ("l_stride_i", C.c_int64),
        ("target", c_f32p), ("t_stride_s", C.c_int64), ("t_stride_h", C.c_int64), ("t_stride_i", C.c_int64),
        ("S", C.c_int64), ("H", C.c_int32), ("G", C.c_int32), ("I", C.c_int64),
        ("Q", C.c_int32), ("Ga", C.c_int32),
        ("taus", C.c_float * TECM_QUANT_MAX_Q),
        ("mean", C.c_double), ("scale", C.c_double),
        ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("clip", C.c_int32), ("_pad2", C.c_int32),
        ("adjust", c_f32p), ("stats", C.c_void_p), ("counts", C.c_void_p), ("group", C.c_void_p), ("err_flag", C.c_void_p),
        ("out_z", c_f32p), ("o_stride_q", C.c_int64), ("o_stride_s", C.c_int64), ("o_stride_h", C.c_int64),
        ("o_stride_i", C.c_int64),
    ]


class TecmQuantileScores(C.Structure):
    _fields_ = [
        ("levels", c_f32p), ("l_stride_q", C.c_int64), ("l_stride_s", C.c_int64), ("l_stride_h", C.c_int64),
        ("l_stride_i", C.c_int64),
        ("target", c_f32p), ("t_stride_s", C.c_int64), ("t_stride_h", C.c_int64), ("t_stride_i", C.c_int64),
        ("S", C.c_int64), ("H", C.c_int32), ("Q", C.c_int32), ("I", C.c_int64),
        ("lo_idx", C.c_int32), ("hi_idx", C.c_int32),
        ("mean", C.c_double), ("scale", C.c_double),
        ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("clip", C.c_int32), ("_pad2", C.c_int32),
        ("scores", c_f32p), ("ld", C.c_int64), ("row0", C.c_int64),
    ]


TECM_COMBINE_MAX_MEMBERS = 8
TECM_COMBINE_EMPTY, TECM_COMBINE_FEW, TECM_COMBINE_DROPPED, TECM_COMBINE_NONFINITE = 1, 2, 4, 8
TECM_COMBINE_PIVOT_TOL = 1e-10


class TecmCombineOperand(C.Structure):
    _fields_ = [("base", c_f32p), ("stride_s", C.c_int64), ("stride_h", C.c_int64), ("stride_i", C.c_int64)]


class TecmCombineMoments(C.Structure):
    _fields_ = [
        ("member", TecmCombineOperand * TECM_COMBINE_MAX_MEMBERS), ("target", TecmCombineOperand),
        ("S", C.c_int64), ("H", C.c_int32), ("G", C.c_int32), ("I", C.c_int64),
        ("M", C.c_int32), ("_pad", C.c_int32),
        ("stats", C.c_void_p), ("group", C.c_void_p), ("err_flag", C.c_void_p),
    ]


class TecmCombineSolve(C.Structure):
    _fields_ = [
        ("stats", C.c_void_p), ("s_stride_g", C.c_int64), ("s_stride_h", C.c_int64), ("s_stride_k", C.c_int64),
        ("s_stride_i", C.c_int64),
        ("G", C.c_int32), ("H", C.c_int32), ("I", C.c_int64),
        ("M", C.c_int32), ("_pad", C.c_int32),
        ("ridge", C.c_double), ("w0", C.c_double * TECM_COMBINE_MAX_MEMBERS),
        ("weight", C.c_void_p), ("intercept", C.c_void_p), ("status", C.c_void_p), ("dropped", C.c_void_p),
    ]


class TecmCombineApply(C.Structure):
    _fields_ = [
        ("member", TecmCombineOperand * TECM_COMBINE_MAX_MEMBERS),
        ("S", C.c_int64), ("H", C.c_int32), ("G", C.c_int32), ("I", C.c_int64),
        ("M", C.c_int32), ("_pad", C.c_int32),
        ("weight", C.c_void_p), ("w_stride_g", C.c_int64), ("w_stride_h", C.c_int64), ("w_stride_m", C.c_int64),
        ("w_stride_i", C.c_int64),
        ("intercept", C.c_void_p), ("b_stride_g", C.c_int64), ("b_stride_h", C.c_int64), ("b_stride_i", C.c_int64),
        ("out", c_f32p), ("o_stride_s", C.c_int64), ("o_stride_h", C.c_int64), ("o_stride_i", C.c_int64),
        ("group", C.c_void_p), ("err_flag", C.c_void_p),
    ]


class TecmMetricsWindow(C.Structure):
    _fields_ = [
        ("pred", c_f32p), ("p_stride_s", C.c_int64), ("p_stride_h", C.c_int64), ("p_stride_i", C.c_int64),
        ("target", c_f32p), ("t_stride_s", C.c_int64), ("t_stride_h", C.c_int64), ("t_stride_i", C.c_int64),
        ("S", C.c_int64), ("H", C.c_int32), ("_pad", C.c_int32), ("I", C.c_int64),
        ("mean", C.c_double), ("scale", C.c_double),
        ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("clip", C.c_int32), ("_pad2", C.c_int32),
        ("table", C.c_void_p), ("table_rows", C.c_int64), ("rows", C.c_void_p), ("row0", C.c_int64),
        ("err_flag", C.c_void_p),
    ]


class TecmBlockBootstrap(C.Structure):
    _fields_ = [
        ("table", C.c_void_p), ("stride_m", C.c_int64), ("stride_s", C.c_int64),
        ("M", C.c_int64), ("S", C.c_int64), ("W", C.c_int64),
        ("group", C.c_void_p), ("G", C.c_int32), ("_pad", C.c_int32),
        ("starts", C.c_void_p), ("R", C.c_int64), ("K", C.c_int64), ("L", C.c_int64),
        ("out", C.c_void_p), ("err_flag", C.c_void_p),
    ]


class TecmEventHist(C.Structure):
    _fields_ = [
        ("members", c_f32p), ("m_stride_k", C.c_int64), ("m_stride_s", C.c_int64), ("m_stride_h", C.c_int64),
        ("m_stride_i", C.c_int64),
        ("target", c_f32p), ("t_stride_s", C.c_int64), ("t_stride_h", C.c_int64), ("t_stride_i", C.c_int64),
        ("S", C.c_int64), ("H", C.c_int32), ("G", C.c_int32), ("I", C.c_int64),
        ("K", C.c_int32), ("Q", C.c_int32),
        ("mean", C.c_double), ("scale", C.c_double),
        ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("clip", C.c_int32), ("num_slots", C.c_int32),
        ("thr", c_f32p), ("th_stride_q", C.c_int64), ("th_stride_k", C.c_int64), ("th_stride_i", C.c_int64),
        ("slot", C.c_void_p),
        ("dir", C.c_int32 * 8),
        ("hist", C.c_void_p), ("group", C.c_void_p), ("err_flag", C.c_void_p),
    ]


class TecmEventFss(C.Structure):
    _fields_ = [
        ("pred", c_f32p), ("p_stride_s", C.c_int64), ("p_stride_h", C.c_int64), ("p_stride_i", C.c_int64),
        ("target", c_f32p), ("t_stride_s", C.c_int64), ("t_stride_h", C.c_int64), ("t_stride_i", C.c_int64),
        ("S", C.c_int64), ("H", C.c_int32), ("G", C.c_int32), ("I", C.c_int64),
        ("rows", C.c_int32), ("cols", C.c_int32), ("Q", C.c_int32), ("W", C.c_int32),
        ("mean", C.c_double), ("scale", C.c_double),
        ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("clip", C.c_int32), ("num_slots", C.c_int32),
        ("thr", c_f32p), ("th_stride_q", C.c_int64), ("th_stride_k", C.c_int64), ("th_stride_i", C.c_int64),
        ("slot", C.c_void_p),
        ("dir", C.c_int32 * 8), ("widths", C.c_int32 * 8),
        ("sums", C.c_void_p), ("group", C.c_void_p), ("err_flag", C.c_void_p),
    ]


class TecmWindowBatch(C.Structure):
    _fields_ = [
        ("X", c_f32p), ("TF", c_f32p), ("Y", c_f32p), ("starts", C.c_void_p), ("starts_host_check", C.c_void_p),
        ("T", C.c_int64), ("row", C.c_int64),
        ("N", C.c_int32), ("L_in", C.c_int32), ("L_out", C.c_int32), ("F_t", C.c_int32), ("B", C.c_int32),
        ("_pad", C.c_int32),
        ("x_out", c_f32p), ("tf_out", c_f32p), ("y_out", c_f32p),
    ]


class TecmWindowBaseline(C.Structure):
    _fields_ = [
        ("X", c_f32p), ("starts", C.c_void_p), ("starts_host_check", C.c_void_p),
        ("T", C.c_int64),
        ("N", C.c_int32), ("C", C.c_int32), ("channel", C.c_int32), ("L_in", C.c_int32), ("L_out", C.c_int32),
        ("B", C.c_int32), ("mode", C.c_int32), ("period", C.c_int32),
        ("out", c_f32p), ("o_stride_b", C.c_int64), ("o_stride_h", C.c_int64), ("o_stride_n", C.c_int64),
    ]


class TecmSlotMean(C.Structure):
    _fields_ = [
        ("x", c_f32p), ("stride_t", C.c_int64), ("stride_n", C.c_int64),
        ("slot", C.c_void_p),
        ("T", C.c_int64), ("N", C.c_int32), ("n_slots", C.c_int32),
        ("means", C.c_void_p), ("counts", C.c_void_p),
    ]


class TecmSarFit(C.Structure):
    _fields_ = [
        ("x", c_f32p), ("stride_t", C.c_int64), ("stride_n", C.c_int64),
        ("T", C.c_int64),
        ("N", C.c_int32), ("d", C.c_int32), ("D", C.c_int32), ("s", C.c_int32), ("m", C.c_int32), ("n_ar", C.c_int32),
        ("n_ma", C.c_int32), ("_pad", C.c_int32),
        ("ar_lags", C.c_int32 * 12), ("ma_lags", C.c_int32 * 12),
        ("autocov", C.c_void_p), ("gram", C.c_void_p), ("wss", C.c_void_p), ("coef", C.c_void_p), ("sigma2", C.c_void_p),
        ("status", C.c_void_p), ("use_ma", C.c_void_p), ("ws", C.c_void_p),
    ]


class TecmSarForecast(C.Structure):
    _fields_ = [
        ("w", TecmWindowBaseline),
        ("coef", C.c_void_p),
        ("d", C.c_int32), ("D", C.c_int32), ("s", C.c_int32), ("n_ar", C.c_int32), ("n_ma", C.c_int32), ("_pad", C.c_int32),
        ("ar_lags", C.c_int32 * 12), ("ma_lags", C.c_int32 * 12),
    ]


class TecmLinGram(C.Structure):
    _fields_ = [
        ("X", c_f32p), ("T", C.c_int64),
        ("ys", c_f32p), ("ys_stride_t", C.c_int64), ("ys_stride_n", C.c_int64), ("Ty", C.c_int64),
        ("N", C.c_int32), ("C", C.c_int32), ("P", C.c_int32), ("H", C.c_int32), ("L_in", C.c_int32), ("pooled", C.c_int32),
        ("chan", C.c_int32 * 64), ("lag", C.c_int32 * 64),
        ("first", C.c_int64), ("step", C.c_int64), ("count", C.c_int64),
        ("gram", C.c_void_p), ("gram_pooled", C.c_void_p),
    ]


class TecmLinSolve(C.Structure):
    _fields_ = [
        ("gram", C.c_void_p),
        ("N", C.c_int32), ("P", C.c_int32), ("H", C.c_int32), ("_pad", C.c_int32),
        ("alpha", C.c_double),
        ("coef", C.c_void_p), ("coef_t", C.c_void_p),
        ("status", C.c_void_p),
    ]


class TecmLinForecast(C.Structure):
    _fields_ = [
        ("w", TecmWindowBaseline),
        ("coef", C.c_void_p), ("coef_stride_n", C.c_int64),
        ("P", C.c_int32), ("_pad", C.c_int32),
        ("chan", C.c_int32 * 64), ("lag", C.c_int32 * 64),
    ]


class TecmAnalogSearch(C.Structure):
    _fields_ = [
        ("A", c_f32p), ("Ta", C.c_int64), ("Ty", C.c_int64),
        ("Xq", c_f32p), ("Tq", C.c_int64),
        ("starts", C.c_void_p), ("starts_host_check", C.c_void_p),
        ("origin_shift", C.c_int64),
        ("N", C.c_int32), ("C", C.c_int32), ("channel", C.c_int32), ("L_in", C.c_int32), ("L_out", C.c_int32),
        ("m", C.c_int32), ("K", C.c_int32), ("S", C.c_int32),
        ("key_arch", C.c_void_p), ("Tk", C.c_int64), ("key_q", C.c_void_p),
        ("exclude", C.c_int32), ("_pad", C.c_int32),
        ("idx", C.c_void_p), ("dist", c_f32p), ("count", C.c_void_p),
    ]


class TecmAnalogForecast(C.Structure):
    _fields_ = [
        ("Y", c_f32p), ("Ty", C.c_int64),
        ("idx", C.c_void_p), ("count", C.c_void_p),
        ("N", C.c_int32), ("K", C.c_int32), ("m", C.c_int32), ("L_out", C.c_int32), ("B", C.c_int32), ("_pad", C.c_int32),
        ("out", c_f32p), ("o_stride_b", C.c_int64), ("o_stride_h", C.c_int64), ("o_stride_n", C.c_int64),
        ("members", c_f32p),
    ]


class TecmFieldScores(C.Structure):
    _fields_ = [
        ("members", c_f32p), ("m_stride_k", C.c_int64), ("m_stride_s", C.c_int64), ("m_stride_h", C.c_int64),
        ("m_stride_i", C.c_int64),
        ("target", c_f32p), ("t_stride_s", C.c_int64), ("t_stride_h", C.c_int64), ("t_stride_i", C.c_int64),
        ("S", C.c_int64), ("H", C.c_int32), ("G", C.c_int32), ("I", C.c_int64),
        ("K", C.c_int32), ("NB", C.c_int32),
        ("mean", C.c_double), ("scale", C.c_double),
        ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("clip", C.c_int32), ("order", C.c_int32),
        ("pair_class", C.c_void_p),
        ("es_stats", C.c_void_p), ("vs_stats", C.c_void_p), ("es_out", C.c_void_p), ("vs_out", C.c_void_p),
        ("group", C.c_void_p), ("err_flag", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class TecmMemberReorder(C.Structure):
    _fields_ = [
        ("values", c_f32p), ("v_stride_k", C.c_int64), ("v_stride_s", C.c_int64), ("v_stride_h", C.c_int64),
        ("v_stride_i", C.c_int64),
        ("tmpl", c_f32p), ("t_stride_k", C.c_int64), ("t_stride_s", C.c_int64), ("t_stride_h", C.c_int64),
        ("t_stride_i", C.c_int64),
        ("rows", C.c_void_p), ("t_stride_row", C.c_int64), ("T", C.c_int64),
        ("out", c_f32p), ("o_stride_k", C.c_int64), ("o_stride_s", C.c_int64), ("o_stride_h", C.c_int64),
        ("o_stride_i", C.c_int64),
        ("out_rank", C.c_void_p),
        ("S", C.c_int64), ("H", C.c_int32), ("K", C.c_int32), ("I", C.c_int64),
        ("err_flag", C.c_void_p),
    ]


class TecmMoments(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("rows", C.c_int64), ("cols", C.c_int64), ("ld", C.c_int64),
        ("src_f64", C.c_int32), ("pool", C.c_int32), ("taps", C.c_int32), ("_pad", C.c_int32),
        ("count", C.c_void_p), ("mean", C.c_void_p), ("var", C.c_void_p),
        ("ws", C.c_void_p),
    ]


class TecmFeaturesBuild(C.Structure):
    _fields_ = [
        ("tec", C.c_void_p), ("idx", C.c_void_p),
        ("rows", C.c_int64), ("x_rows", C.c_int64), ("N", C.c_int32), ("Ci", C.c_int32), ("H", C.c_int32),
        ("tec_f64", C.c_int32), ("idx_f64", C.c_int32), ("_pad", C.c_int32),
        ("mean", C.POINTER(C.c_double)), ("scale", C.POINTER(C.c_double)),
        ("ymean", C.c_double), ("yscale", C.c_double),
        ("X", c_f32p), ("Ys", c_f32p), ("Y", c_f32p),
    ]


class TecmWindowBatchSeries(C.Structure):
    _fields_ = [
        ("X", c_f32p), ("TF", c_f32p), ("Ys", c_f32p), ("starts", C.c_void_p), ("starts_host_check", C.c_void_p),
        ("T", C.c_int64), ("Ty", C.c_int64), ("row", C.c_int64),
        ("N", C.c_int32), ("L_in", C.c_int32), ("L_out", C.c_int32), ("F_t", C.c_int32), ("B", C.c_int32),
        ("_pad", C.c_int32),
        ("x_out", c_f32p), ("tf_out", c_f32p), ("y_out", c_f32p),
    ]


class TecmConvDx(C.Structure):
    _fields_ = [("dy", C.c_void_p), ("wpack", C.c_void_p), ("dinp", c_f32p),
                ("B", C.c_int32), ("Lc", C.c_int32), ("N", C.c_int32), ("Cout", C.c_int32), ("ld_in", C.c_int32),
                ("_pad", C.c_int32)]


class TecmConvDw(C.Structure):
    _fields_ = [("inp", C.c_void_p), ("dy", C.c_void_p), ("workspace", c_f32p), ("dw3", c_f32p), ("dw5", c_f32p),
                ("dw7", c_f32p),
                ("B", C.c_int32), ("Lc", C.c_int32), ("N", C.c_int32), ("Cout", C.c_int32), ("Cin", C.c_int32),
                ("ld_in", C.c_int32), ("num_blocks", C.c_int32), ("_pad", C.c_int32)]


class TecmConvFwd(C.Structure):
    _fields_ = [("inp", C.c_void_p), ("wpack", C.c_void_p), ("bias", c_f32p), ("y", c_f32p),
                ("B", C.c_int32), ("Lc", C.c_int32), ("N", C.c_int32), ("Cout", C.c_int32), ("ld_in", C.c_int32),
                ("y_bf16", C.c_int32), ("stats", c_f32p), ("eps", C.c_float), ("_pad", C.c_int32)]


TECM_NORM_BLOCKS = 512
TECM_METRIC_STATS = 8
TECM_MAP_LDS_MAX_H = 32
TECM_ENS_STATS = 9
TECM_ENS_MAX_K = 64
TECM_CONF_ABS, TECM_CONF_SIGNED = 0, 1
TECM_INTERVAL_STATS = 6
TECM_SELECT_MAX_Q = 8
TECM_BAD_ROW, TECM_BAD_START = 32, 64
TECM_BAD_SLOT = 128
TECM_EVENT_MAX_Q, TECM_EVENT_MAX_W, TECM_EVENT_LDS_WORDS = 8, 8, 256
TECM_ATTN_SKIP_UNCONNECTED = 1
TECM_TATT_COUNT = 8
TECM_BASELINE_MEAN, TECM_BASELINE_LAST, TECM_BASELINE_PERIODIC = 0, 1, 2
TECM_SAR_MAX_K, TECM_SAR_MAX_LAG, TECM_SAR_MAX_LONG_AR, TECM_SAR_MAX_OFFSET, TECM_SAR_CHUNK = 12, 32, 64, 64, 1024
TECM_SAR_DEGENERATE, TECM_SAR_NONFINITE, TECM_SAR_MA_DROPPED = 1, 2, 4
TECM_LIN_MAX_P, TECM_LIN_MAX_H, TECM_LIN_MAX_LAG, TECM_LIN_MAX_CHANNELS = 64, 32, 512, 8
TECM_LIN_DEGENERATE, TECM_LIN_NONFINITE = 1, 2
TECM_ANALOG_MAX_K, TECM_ANALOG_MAX_M, TECM_ANALOG_MAX_H = 32, 512, 32
TECM_MOMENTS_MAX_BLOCKS = 2048
TECM_FIELD_ORDER_HALF, TECM_FIELD_ORDER_ONE, TECM_FIELD_ORDER_TWO = 0, 1, 2
TECM_FIELD_MAX_CLASSES, TECM_FIELD_ES_STATS, TECM_FIELD_VS_STATS = 16, 4, 5
TECM_FIELD_MAX_GRID, TECM_FIELD_MAX_TILES = 65535, 65535
TECM_REORDER_MAX_GRID = 65535
TECM_FEATURES_MAX_CI = 15


EXPORTS = {
    "tecm_abi_version": (C.c_int, []),
    "tecm_last_error": (C.c_char_p, []),
    "tecm_gemm_f32": (C.c_int, [C.POINTER(TecmGemm), C.c_void_p]),
    "tecm_gemm_bf16": (C.c_int, [C.POINTER(TecmGemm), C.c_void_p]),
    "tecm_gemm_bf16x3": (C.c_int, [C.POINTER(TecmGemm), C.c_void_p]),
    "tecm_gemm_bf16x6": (C.c_int, [C.POINTER(TecmGemm), C.c_void_p]),
    "tecm_gemm_last_kernel": (C.c_char_p, []),
    "tecm_gemm_last_skipped_flops": (C.c_int64, []),
    "tecm_gemm_rows_in_rect": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "tecm_gemm_rect_tiles": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "tecm_attention_reads_q0": (C.c_int, [C.c_int32]),
    "tecm_spatial_fwd_lds_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "tecm_spatial_bwd_lds_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "tecm_spatial_fwd": (C.c_int, [C.POINTER(TecmSpatial), C.c_void_p]),
    "tecm_spatial_fwd2_ws_floats": (C.c_int64, [C.POINTER(TecmSpatial)]),
    "tecm_spatial_fwd2": (C.c_int, [C.POINTER(TecmSpatial), c_f32p, C.c_void_p]),
    "tecm_spatial_bwd": (C.c_int, [C.POINTER(TecmSpatial), C.POINTER(TecmSpatialGrads), C.c_void_p]),
    "tecm_spatial_bwd_blocks": (C.c_int, [C.POINTER(TecmSpatial)]),
    "tecm_spatial_bwd2_blocks": (C.c_int, [C.POINTER(TecmSpatial)]),
    "tecm_spatial_bwd2": (C.c_int, [C.POINTER(TecmSpatial), C.POINTER(TecmSpatialGrads), c_f32p, C.c_void_p]),
    "tecm_spatial_dx_ws_floats": (C.c_int64, [C.POINTER(TecmSpatial)]),
    "tecm_spatial_dx": (C.c_int, [C.POINTER(TecmSpatial), C.POINTER(TecmSpatialDx), C.c_void_p]),
    "tecm_spatial_attention_ws_floats": (C.c_int64, [C.POINTER(TecmSpatial), C.POINTER(TecmSpatialAttn)]),
    "tecm_spatial_attention": (C.c_int, [C.POINTER(TecmSpatial), C.POINTER(TecmSpatialAttn), C.c_void_p]),
    "tecm_temporal_attention_ws_floats": (C.c_int64, [C.POINTER(TecmTemporalAttn)]),
    "tecm_temporal_attention": (C.c_int, [C.POINTER(TecmTemporalAttn), C.c_void_p]),
    "tecm_groupnorm_gelu_fwd": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_void_p]),
    "tecm_gn_y16_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "tecm_gn_reg_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "tecm_gn_fwd_path": (C.c_char_p, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "tecm_gn_bwd_path": (C.c_char_p, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "tecm_groupnorm_gelu_bwd": (C.c_int, [c_f32p, C.c_int32, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                          C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, c_f32p, C.c_void_p]),
    "tecm_layernorm_fwd": (C.c_int, [c_f32p, C.c_int64, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_int64, C.POINTER(TecmDrop), C.c_int32, C.c_int32, C.c_int32,
                                     c_f32p, C.c_int64, C.c_int32, C.c_float, C.c_void_p]),
    "tecm_layernorm_bwd": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p,
                                     C.c_int32, C.POINTER(TecmDrop), c_f32p, C.POINTER(C.c_int32), C.c_int64, C.c_int32,
                                     C.POINTER(TecmLnAdd), C.c_int32, C.POINTER(TecmLnDyMap), C.c_int32, C.c_void_p]),
    "tecm_attention_fwd": (C.c_int, [c_f32p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.POINTER(TecmDrop), C.c_void_p]),
    "tecm_cast_bf16": (C.c_int, [c_f32p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
    "tecm_attention_bwd": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.POINTER(TecmDrop), C.c_void_p]),
    "tecm_colsum": (C.c_int, [c_f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, c_f32p, C.c_int64,
                              C.c_int32, C.c_float, C.POINTER(TecmDrop), c_f32p, C.c_void_p]),
    "tecm_colsum_twin": (C.c_int, [c_f32p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, c_f32p, C.c_int64,
                                   C.c_int32, C.c_float, C.POINTER(TecmDrop), c_f32p, C.c_void_p, C.c_int64, C.c_void_p]),
    "tecm_colsum_batch": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                                    c_f32p, C.c_void_p]),
    "tecm_colsum_path": (C.c_char_p, [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "tecm_huber_fwd_bwd":(C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_float, C.c_float, c_f32p,
                                     C.c_void_p]),
    "tecm_huber_fwd_bwd_strided": (C.c_int, [c_f32p, C.POINTER(C.c_int64), c_f32p, C.POINTER(C.c_int64), c_f32p, c_f32p,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, c_f32p, C.c_void_p]),
    "tecm_lora_fold": (C.c_int, [c_f32p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                 C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "tecm_pack_vectors": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32, c_f32p, C.c_void_p]),
    "tecm_conv_weight_pack": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "tecm_conv_weight_unpack": (C.c_int, [c_f32p, c_f32p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "tecm_conv_dx_pack": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "tecm_conv_dx_bf16": (C.c_int, [C.POINTER(TecmConvDx), C.c_void_p]),
    "tecm_conv_fwd_pack": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "tecm_conv_fwd_bf16": (C.c_int, [C.POINTER(TecmConvFwd), C.c_void_p]),
    "tecm_conv_fwd_pack_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "tecm_conv_fwd_f32": (C.c_int, [C.POINTER(TecmConvFwd), C.c_void_p]),
    "tecm_conv_dw_workspace": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "tecm_conv_dw_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "tecm_conv_dw_bf16": (C.c_int, [C.POINTER(TecmConvDw), C.c_void_p]),
    "tecm_conv_dw_f32": (C.c_int, [C.POINTER(TecmConvDw), C.c_void_p]),
    "tecm_conv_dx_pack_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "tecm_conv_dx_f32": (C.c_int, [C.POINTER(TecmConvDx), C.c_void_p]),
    "tecm_conv_fwd_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "tecm_conv_fwd_stats_supported": (C.c_int, [C.c_int32]),
    "tecm_gemm_tn_splits": (C.c_int32, [C.c_int64, C.c_int64, C.c_int64]),
    "tecm_p8_rows": (C.c_int, [C.c_int64, C.c_int64]),
    "tecm_gemm_tile_of_block": (None, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "tecm_gemm_tiles_of_blocks": (None, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "tecm_conv_dx_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "tecm_conv_fwd_tile_steps": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "tecm_conv_dx_tile_steps": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "tecm_transpose_scale": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_int32, C.c_int32, C.c_float,
                                       C.c_void_p]),
    "tecm_weight_bf16": (C.c_int, [c_f32p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                   C.c_void_p]),
    "tecm_dropout_apply": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                     C.c_int32, C.POINTER(TecmDrop), C.c_void_p]),
    "tecm_adamw_clip_step": (C.c_int, [C.POINTER(TecmAdamW), C.c_void_p]),
    "tecm_checksum_tail": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "tecm_checksum_verify": (C.c_int, [c_f32p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "tecm_seed_advance": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "tecm_metrics_accumulate": (C.c_int, [C.POINTER(TecmMetrics), C.c_void_p]),
    "tecm_metrics_map": (C.c_int, [C.POINTER(TecmMetricsMap), C.c_void_p]),
    "tecm_ensemble_stats": (C.c_int, [C.POINTER(TecmEnsemble), C.c_void_p]),
    "tecm_event_hist": (C.c_int, [C.POINTER(TecmEventHist), C.c_void_p]),
    "tecm_event_fss": (C.c_int, [C.POINTER(TecmEventFss), C.c_void_p]),
    "tecm_event_fss_supported": (C.c_int, [C.c_int32, C.c_int32]),
    "tecm_conformal_scores": (C.c_int, [C.POINTER(TecmConformalScores), C.c_void_p]),
    "tecm_column_select": (C.c_int, [C.POINTER(TecmColumnSelect), C.c_void_p]),
    "tecm_interval_stats": (C.c_int, [C.POINTER(TecmIntervalStats), C.c_void_p]),
    "tecm_pinball_fwd_bwd_strided": (C.c_int, [C.POINTER(TecmPinball), C.c_void_p]),
    "tecm_quantile_stats": (C.c_int, [C.POINTER(TecmQuantileStats), C.c_void_p]),
    "tecm_quantile_scores": (C.c_int, [C.POINTER(TecmQuantileScores), C.c_void_p]),
    "tecm_combine_moments": (C.c_int, [C.POINTER(TecmCombineMoments), C.c_void_p]),
    "tecm_combine_solve": (C.c_int, [C.POINTER(TecmCombineSolve), C.c_void_p]),
    "tecm_combine_apply": (C.c_int, [C.POINTER(TecmCombineApply), C.c_void_p]),
    "tecm_metrics_window": (C.c_int, [C.POINTER(TecmMetricsWindow), C.c_void_p]),
    "tecm_block_bootstrap": (C.c_int, [C.POINTER(TecmBlockBootstrap), C.c_void_p]),
    "tecm_window_batch": (C.c_int, [C.POINTER(TecmWindowBatch), C.c_void_p]),
    "tecm_window_baseline": (C.c_int, [C.POINTER(TecmWindowBaseline), C.c_void_p]),
    "tecm_slot_mean": (C.c_int, [C.POINTER(TecmSlotMean), C.c_void_p]),
    "tecm_sar_fit_ws_bytes": (C.c_int64, [C.POINTER(TecmSarFit)]),
    "tecm_sar_fit": (C.c_int, [C.POINTER(TecmSarFit), C.c_void_p]),
    "tecm_sar_solve": (C.c_int, [C.POINTER(TecmSarFit), C.c_void_p]),
    "tecm_sar_forecast": (C.c_int, [C.POINTER(TecmSarForecast), C.c_void_p]),
    "tecm_lin_gram_supported": (C.c_int, [C.POINTER(TecmLinGram), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tecm_lin_gram": (C.c_int, [C.POINTER(TecmLinGram), C.c_void_p]),
    "tecm_lin_solve": (C.c_int, [C.POINTER(TecmLinSolve), C.c_void_p]),
    "tecm_lin_forecast": (C.c_int, [C.POINTER(TecmLinForecast), C.c_void_p]),
    "tecm_analog_search_supported": (C.c_int, [C.POINTER(TecmAnalogSearch), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                               C.POINTER(C.c_int64)]),
    "tecm_analog_search": (C.c_int, [C.POINTER(TecmAnalogSearch), C.c_void_p]),
    "tecm_analog_forecast": (C.c_int, [C.POINTER(TecmAnalogForecast), C.c_void_p]),
    "tecm_field_scores_plan": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tecm_field_scores": (C.c_int, [C.POINTER(TecmFieldScores), C.c_void_p]),
    "tecm_member_reorder": (C.c_int, [C.POINTER(TecmMemberReorder), C.c_void_p]),
    "tecm_moments_ws_bytes": (C.c_int64, [C.POINTER(TecmMoments)]),
    "tecm_moments": (C.c_int, [C.POINTER(TecmMoments), C.c_void_p]),
    "tecm_features_build": (C.c_int, [C.POINTER(TecmFeaturesBuild), C.c_void_p]),
    "tecm_window_batch_series": (C.c_int, [C.POINTER(TecmWindowBatchSeries), C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


class TecmError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load the HIP library once.  No fallback: a missing/incompatible library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TecmError(
            f"{LIB_PATH} not found: build it first (python -c 'import __graft_entry__ as g; g.build()'). "
            "The TEC-MoLLM MI355X path has no CPU/PyTorch fallback.")
    handle = C.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(handle, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if handle.tecm_abi_version() != ABI_VERSION:
        raise TecmError(f"ABI mismatch: library {handle.tecm_abi_version()} != binding {ABI_VERSION}")
    _lib = handle
    return handle


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().tecm_last_error().decode("utf-8", "replace")
        raise TecmError(f"{what or 'tecm call'} failed (code {rc}): {msg}")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def require_gpu_tensor(t: torch.Tensor, name: str, dtype=torch.float32) -> None:
    if not t.is_cuda:
        raise TecmError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise TecmError(f"{name} must be {dtype} (got {t.dtype})")
