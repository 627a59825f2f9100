"""Device-side mirror of the reference's `src/models/baselines.py` (`HistoricalAverage`, `save_baseline`,
`load_baseline`).

`HistoricalAverage.fit` (:13-33) loops over nodes x 12 slots on the host with one masked `np.mean` each; here one
kernel (`tecm_slot_mean`) returns the (N, 12) table from a series that already lives on the device: fp64 sums in a fixed
order, so the table does not depend on the launch.  The series is read as float32, the dtype the processed splits
carry; a float64 input is rounded to it first.  `predict` (:35-45) is a row gather.

`SarimaBaseline` (:47-72) keeps the reference's constructor and its two methods, but NOT its estimator.  The reference
wraps statsmodels' SARIMAX: an exact Gaussian likelihood of the multiplicative model, maximised iteratively on the host,
one node at a time.  Here the model is the SUBSET (additive) seasonal ARMA on the differenced series -- every lag of the
expanded product polynomials carries a free coefficient, so the default (1,1,1)(1,1,1,12) has AR and MA lags {1, 12, 13}
with three free coefficients each where the multiplicative model ties the third to the product of the other two -- and
it is estimated by the two-stage Hannan-Rissanen regression: a long autoregression (Levinson-Durbin on the sample
autocovariances) supplies innovation estimates, and one least-squares solve on lagged values and lagged innovations gives
the coefficients.  All linear algebra in fp64, no iteration, no constant term; every node of a split is fitted by one
call (`tecm_sar_fit`), and every window of a test split is forecast by one launch (`tecm_sar_forecast`), which the
reference's class cannot do at all (it forecasts from the end of the training series only).  The estimates are
consistent but not the maximum-likelihood ones: expect coefficients and forecasts close to, not equal to, statsmodels'.

`LinearBaseline` is not in the reference: a direct linear map from the input window to the L_out targets, fitted per node
by ridge regression against the TARGET-scaled series -- the "Linear" baseline an LLM-based forecaster is asked to beat.
The normal equations of every window of a split are accumulated on the device (`tecm_lin_gram`), solved by Cholesky
(`tecm_lin_solve`), and every window of a test split is forecast by one launch (`tecm_lin_forecast`).

`AnalogBaseline` is not in the reference either: the analog ensemble, the non-parametric baseline.  For every window and
node the K stretches of the training record nearest to the window's last input steps are searched on the device
(`tecm_analog_search`: the distances are swept and the K best kept in one kernel, no table is stored), and what followed
them is the forecast (`tecm_analog_forecast`): K members, whose spread comes from the data, and their mean.
"""
from __future__ import annotations

import ctypes as C
import logging
import weakref
from typing import Sequence, Union

import numpy as np
import torch

from tecmollm import _lib
from tecmollm._lib import (TecmAnalogForecast, TecmAnalogSearch, TecmLinForecast, TecmLinGram, TecmLinSolve, TecmSarFit, TecmSarForecast, TecmSlotMean,
                           TecmWindowBaseline, check, lib, require_gpu_tensor, stream_ptr)

log = logging.getLogger(__name__)

SLOTS_PER_DAY = 12          # 2-hour resolution (:23)
ArrayLike = Union[np.ndarray, torch.Tensor]


def time_slots(time_data: ArrayLike) -> np.ndarray:
    """The reference's hour-to-slot rule (:26-27, :39-40) on the host: `datetime64[h] % 24 // 2`, int64 in [0, 12).
    Accepts datetime64 values of any unit, or integers counted in hours since the epoch (what `astype('datetime64[h]')`
    makes of them); a tensor is copied to the host first."""
    if isinstance(time_data, torch.Tensor):
        time_data = time_data.cpu().numpy()
    hours = np.asarray(time_data).astype("datetime64[h]").astype(np.int64) % 24
    return hours // 2


def slot_mean(series: torch.Tensor, slots: torch.Tensor, n_slots: int):
    """(T, N) float32 device tensor of any strides + (T) int32 device slots -> ((N, n_slots) float64 means, (n_slots)
    float64 counts), both on the device.  An empty slot gives a NaN column."""
    require_gpu_tensor(series, "series")
    require_gpu_tensor(slots, "slots", torch.int32)
    if series.dim() != 2 or slots.dim() != 1 or slots.shape[0] != series.shape[0]:
        raise ValueError(f"series must be (T, N) and slots (T), got {tuple(series.shape)} and {tuple(slots.shape)}")
    T, N = series.shape
    slots = slots.contiguous()
    means = torch.empty(N, n_slots, device=series.device, dtype=torch.float64)
    counts = torch.empty(n_slots, device=series.device, dtype=torch.float64)
    m = TecmSlotMean(x=series.data_ptr(), stride_t=series.stride(0), stride_n=series.stride(1), slot=slots.data_ptr(),
                     T=T, N=N, n_slots=n_slots, means=means.data_ptr(), counts=counts.data_ptr())
    check(lib().tecm_slot_mean(C.byref(m), stream_ptr()), "tecm_slot_mean")
    return means, counts


class HistoricalAverage:
    def __init__(self, device: Union[str, torch.device] = "cuda"):
        self.averages = None                    # (N, 12) float64 numpy, as in the reference
        self.device = torch.device(device)
        self._table = None                      # the same table on the device, (12, N)

    def __getstate__(self):                      # joblib / pickle: the table only, as the reference's object holds
        return {"averages": self.averages, "device": str(self.device)}

    def __setstate__(self, state):
        self.averages, self.device, self._table = state["averages"], torch.device(state["device"]), None

    def fit(self, tec_data: ArrayLike, time_data: ArrayLike) -> "HistoricalAverage":
        """tec_data (N_times, N_nodes): a numpy array (uploaded once) or a device tensor (read in place, e.g. channel 0
        of a resident split `X.view(T, N, C)[:, :, 0]`); time_data: the matching time stamps (see `time_slots`)."""
        log.info("Fitting Historical Average model...")
        series = tec_data if isinstance(tec_data, torch.Tensor) else torch.as_tensor(np.asarray(tec_data))
        series = series.to(device=self.device if not series.is_cuda else series.device, dtype=torch.float32)
        slots = torch.as_tensor(time_slots(time_data).astype(np.int32)).to(series.device)
        means, _ = slot_mean(series, slots, SLOTS_PER_DAY)
        self._table = means.t().contiguous()
        self.averages = means.cpu().numpy()
        log.info("HA model fitted.")
        return self

    def predict(self, time_data: ArrayLike, num_nodes: int) -> ArrayLike:
        """(len(time_data), num_nodes) float64: row i is the fitted average of slot(time_data[i]) for every node.  A numpy
        array, as the reference returns; a device tensor when `time_data` is one."""
        if self.averages is None:
            raise ValueError("HistoricalAverage.predict() before fit()")
        if self.averages.shape[0] != num_nodes:
            raise ValueError(f"fitted on {self.averages.shape[0]} nodes, asked for {num_nodes}")
        if self._table is None:
            self._table = torch.as_tensor(self.averages).to(self.device).t().contiguous()
        slots = torch.as_tensor(time_slots(time_data)).to(self._table.device)
        pred = self._table.index_select(0, slots)
        return pred if isinstance(time_data, torch.Tensor) and time_data.is_cuda else pred.cpu().numpy()


def sarima_lags(order, seasonal_order, long_ar=None):
    """(p, d, q), (P, D, Q, s) -> (d, D, s, ar_lags, ma_lags, m): the lags of the expanded product polynomials,
    { i + s j : 0 <= i <= p, 0 <= j <= P } without 0 (likewise q, Q), and the order m of the long autoregression
    (default 2 Lmax clipped to [8, 64]).  Raises ValueError outside the ranges the kernels serve."""
    try:
        p, d, q = (int(v) for v in order)
        P, D, Q, s = (int(v) for v in seasonal_order)
    except (TypeError, ValueError):
        raise ValueError(f"order must be (p, d, q) and seasonal_order (P, D, Q, s), got {order!r} and {seasonal_order!r}")
    if min(p, q, P, Q) < 0:
        raise ValueError("p, q, P, Q must not be negative")
    if d not in (0, 1) or D not in (0, 1):
        raise ValueError(f"d and D must be 0 or 1, got d = {d}, D = {D}")
    if (P or Q or D) and s < 1:
        raise ValueError(f"a seasonal term needs a period s >= 1, got {s}")
    if not (P or Q or D):
        s = max(s, 0)
    ar = sorted({i + s * j for i in range(p + 1) for j in range(P + 1)} - {0})
    ma = sorted({i + s * j for i in range(q + 1) for j in range(Q + 1)} - {0})
    K = len(ar) + len(ma)
    if not 1 <= K <= _lib.TECM_SAR_MAX_K:
        raise ValueError(f"the model must have between 1 and {_lib.TECM_SAR_MAX_K} coefficients, this one has {K}")
    lmax = max(ar + ma)
    if lmax > _lib.TECM_SAR_MAX_LAG:
        raise ValueError(f"the largest lag is {lmax}; at most {_lib.TECM_SAR_MAX_LAG} is served")
    if d + s * D > _lib.TECM_SAR_MAX_OFFSET:
        raise ValueError(f"the differencing offset d + s D is {d + s * D}; at most {_lib.TECM_SAR_MAX_OFFSET} is served")
    m = min(max(2 * lmax, 8), _lib.TECM_SAR_MAX_LONG_AR) if long_ar is None else int(long_ar)
    if not lmax <= m <= _lib.TECM_SAR_MAX_LONG_AR:
        raise ValueError(f"long_ar must lie in [{lmax}, {_lib.TECM_SAR_MAX_LONG_AR}], got {m}")
    return d, D, s, ar, ma, m


def ma_invertible(theta: np.ndarray, ma_lags) -> np.ndarray:
    """(N, len(ma_lags)) coefficients -> (N,) bool: every root of 1 + sum_b theta_b z^b lies outside the unit circle, i.e.
    every eigenvalue of the companion matrix of x^L + theta_1 x^(L-1) + ... + theta_L (x = 1 / z) is inside it.  A row
    with a NaN counts as invertible (there is nothing to repair)."""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    ok = np.ones(theta.shape[0], dtype=bool)
    if not len(ma_lags):
        return ok
    L = int(max(ma_lags))
    full = np.zeros((theta.shape[0], L))
    full[:, np.asarray(ma_lags) - 1] = theta
    rows = np.isfinite(full).all(axis=1)
    comp = np.zeros((int(rows.sum()), L, L))
    comp[:, 0, :] = -full[rows]
    comp[:, np.arange(1, L), np.arange(L - 1)] = 1.0
    if comp.shape[0]:
        ok[rows] = np.abs(np.linalg.eigvals(comp)).max(axis=1) < 1.0
    return ok


def _lag_array(lags):
    return (C.c_int32 * 12)(*[int(v) for v in lags])


class SarimaBaseline:
    """The reference's `SarimaBaseline(order, seasonal_order)` with `fit` and `predict`, fitted and forecast on the device
    (see the module docstring for the estimator and how it differs from statsmodels').  After `fit`: `ar_lags`,
    `ma_lags`, `coef_` (N, K) = (phi over ar_lags, theta over ma_lags), `sigma2_` (N), `status_` (N) int32 with the bits
    `DEGENERATE` (zero coefficients: the forecast is the differencing rule alone), `NONFINITE` (NaN coefficients) and
    `MA_DROPPED` (the fitted theta was not invertible; the node was solved again as a pure AR) -- numpy arrays all."""
    DEGENERATE, NONFINITE, MA_DROPPED = _lib.TECM_SAR_DEGENERATE, _lib.TECM_SAR_NONFINITE, _lib.TECM_SAR_MA_DROPPED
    PREDICT_WINDOW = 1024

    def __init__(self, order=(1, 1, 1), seasonal_order=(1, 1, 1, 12), long_ar=None, device: Union[str, torch.device] = "cuda"):
        self.d, self.D, self.s, ar, ma, self.long_ar = sarima_lags(order, seasonal_order, long_ar)
        self.order, self.seasonal_order = tuple(order), tuple(seasonal_order)
        self.ar_lags, self.ma_lags = np.asarray(ar, dtype=np.int32), np.asarray(ma, dtype=np.int32)
        self.device = torch.device(device)
        self.coef_ = self.sigma2_ = self.status_ = self.autocov_ = self.nodes_ = self.tail_ = None
        self._coef_dev = None

    # joblib / pickle: numpy only
    def __getstate__(self):
        state = {k: v for k, v in self.__dict__.items() if k != "_coef_dev"}
        state["device"] = str(self.device)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.device, self._coef_dev = torch.device(state["device"]), None

    @property
    def K(self) -> int:
        return len(self.ar_lags) + len(self.ma_lags)

    @property
    def lmax(self) -> int:
        return int(max(list(self.ar_lags) + list(self.ma_lags)))

    @property
    def offset(self) -> int:
        return self.d + self.s * self.D

    def _fit_desc(self, series, out, use_ma=None, ws=None) -> TecmSarFit:
        return TecmSarFit(x=series.data_ptr(), stride_t=series.stride(0), stride_n=series.stride(1), T=series.shape[0],
                          N=series.shape[1], d=self.d, D=self.D, s=self.s, m=self.long_ar, n_ar=len(self.ar_lags),
                          n_ma=len(self.ma_lags), ar_lags=_lag_array(self.ar_lags), ma_lags=_lag_array(self.ma_lags),
                          autocov=out["autocov"].data_ptr(), gram=out["gram"].data_ptr(), wss=out["wss"].data_ptr(),
                          coef=out["coef"].data_ptr(), sigma2=out["sigma2"].data_ptr(), status=out["status"].data_ptr(),
                          use_ma=None if use_ma is None else use_ma.data_ptr(), ws=None if ws is None else ws.data_ptr())

    def fit_device(self, series: torch.Tensor):
        """Stage 1 and 2 on a (T, N) float32 device tensor of any non-negative strides: a dict of device tensors `autocov`
        (N, m+1), `gram` (N, K, K+1), `wss` (N), `coef` (N, K), `sigma2` (N), all float64, and `status` (N) int32 --
        what `tecm_sar_fit` writes, before the invertibility repair of `fit`."""
        require_gpu_tensor(series, "series")
        if series.dim() != 2:
            raise ValueError(f"series must be (T, N), got {tuple(series.shape)}")
        N, K, f64 = series.shape[1], self.K, dict(device=series.device, dtype=torch.float64)
        out = {"autocov": torch.empty(N, self.long_ar + 1, **f64), "gram": torch.empty(N, K, K + 1, **f64),
               "wss": torch.empty(N, **f64), "coef": torch.empty(N, K, **f64), "sigma2": torch.empty(N, **f64),
               "status": torch.empty(N, device=series.device, dtype=torch.int32)}
        desc = self._fit_desc(series, out)
        nbytes = lib().tecm_sar_fit_ws_bytes(C.byref(desc))
        if nbytes < 0:
            check(1, "tecm_sar_fit_ws_bytes")
        ws = torch.empty(nbytes // 8, **f64)
        desc = self._fit_desc(series, out, ws=ws)
        check(lib().tecm_sar_fit(C.byref(desc), stream_ptr()), "tecm_sar_fit")
        return out

    def solve_device(self, series: torch.Tensor, out, use_ma: torch.Tensor) -> None:
        """Solves the nodes with `use_ma[node] == 0` again from `out["gram"]` as pure AR models (theta = 0), in place."""
        require_gpu_tensor(use_ma, "use_ma", torch.int8)
        if use_ma.shape != (series.shape[1],):
            raise ValueError(f"use_ma must hold one flag per node ({series.shape[1]})")
        desc = self._fit_desc(series, out, use_ma=use_ma.contiguous())
        check(lib().tecm_sar_solve(C.byref(desc), stream_ptr()), "tecm_sar_solve")

    def fit(self, tec_data: ArrayLike, node_indices=None) -> "SarimaBaseline":
        """tec_data (N_times, N_nodes): a numpy array (uploaded once) or a device tensor (read in place, e.g. channel 0 of
        a resident split).  `node_indices` None fits every node; a list fits those columns only, as the reference does.
        One host synchronisation: theta is checked for invertibility with numpy and the nodes that fail are solved
        again without their MA part (`MA_DROPPED`)."""
        series = tec_data if isinstance(tec_data, torch.Tensor) else torch.as_tensor(np.asarray(tec_data))
        series = series.to(device=self.device if not series.is_cuda else series.device, dtype=torch.float32)
        if series.dim() != 2:
            raise ValueError(f"tec_data must be (N_times, N_nodes), got {tuple(series.shape)}")
        if node_indices is None:
            nodes = np.arange(series.shape[1], dtype=np.int64)
        else:
            nodes = np.asarray([int(i) for i in node_indices], dtype=np.int64)
            series = series.index_select(1, torch.as_tensor(nodes).to(series.device))
        log.info("Fitting SARIMA (Hannan-Rissanen) for %d nodes...", len(nodes))
        out = self.fit_device(series)
        n_ar = len(self.ar_lags)
        theta = out["coef"][:, n_ar:].cpu().numpy()
        bad = ~ma_invertible(theta, self.ma_lags)
        if bad.any():
            use_ma = torch.as_tensor((~bad).astype(np.int8)).to(series.device)
            self.solve_device(series, out, use_ma)
        self._coef_dev = out["coef"]
        self.coef_, self.sigma2_ = out["coef"].cpu().numpy(), out["sigma2"].cpu().numpy()
        self.status_, self.autocov_ = out["status"].cpu().numpy(), out["autocov"].cpu().numpy()
        self.nodes_ = nodes
        self.tail_ = series[-min(series.shape[0], self.PREDICT_WINDOW):].contiguous().cpu().numpy()
        log.info("SARIMA fitted: %d degenerate, %d non-finite, %d without MA part.", int((self.status_ & 1 != 0).sum()),
                 int((self.status_ & 2 != 0).sum()), int((self.status_ & 4 != 0).sum()))
        return self

    def _coef_on(self, device) -> torch.Tensor:
        if self.coef_ is None:
            raise ValueError("SarimaBaseline used before fit()")
        if self._coef_dev is None or self._coef_dev.device != device:
            self._coef_dev = torch.as_tensor(self.coef_).to(device).contiguous()
        return self._coef_dev

    def forecast_series(self, X: torch.Tensor, starts: Sequence[int], L_in: int, L_out: int, channel: int = 0,
                        out: torch.Tensor = None, coef: torch.Tensor = None, host_check: bool = True) -> torch.Tensor:
        """Forecasts from the windows X[a : a + L_in, :, channel], a in `starts`, of a (T, N, C) float32 device tensor:
        (B, L_out, N) float32, or written into `out` (any strides).  `coef` (N, K) float64 on the device replaces the
        fitted coefficients.  Without `host_check` a window outside [0, T - L_in] reaches the kernel, which writes NaN."""
        require_gpu_tensor(X, "X")
        if X.dim() != 3 or not X.is_contiguous():
            raise ValueError(f"X must be a contiguous (T, N, C) tensor, got {tuple(X.shape)}")
        T, N, Cc = X.shape
        need = self.offset + self.lmax + 1
        if L_in < need:
            raise ValueError(f"L_in = {L_in} is shorter than d + s D + Lmax + 1 = {need}")
        coef = self._coef_on(X.device) if coef is None else coef
        require_gpu_tensor(coef, "coef", torch.float64)
        if coef.shape != (N, self.K) or not coef.is_contiguous():
            raise ValueError(f"coefficients of shape {tuple(coef.shape)} do not fit {N} nodes x {self.K} lags")
        host = torch.tensor([int(a) for a in starts], dtype=torch.int64)
        B = host.numel()
        if B == 0:
            raise ValueError("forecast_series() needs at least one window")
        if out is None:
            out = torch.empty(B, int(L_out), N, device=X.device, dtype=torch.float32)
        require_gpu_tensor(out, "out")
        if out.shape != (B, int(L_out), N):
            raise ValueError(f"out must be {(B, int(L_out), N)}, got {tuple(out.shape)}")
        dev_starts = host.to(X.device, non_blocking=True)
        w = TecmWindowBaseline(X=X.data_ptr(), starts=dev_starts.data_ptr(), starts_host_check=host.data_ptr() if host_check else None, T=T, N=N,
                               C=Cc, channel=int(channel), L_in=int(L_in), L_out=int(L_out), B=B, mode=0, period=0,
                               out=out.data_ptr(), o_stride_b=out.stride(0), o_stride_h=out.stride(1) if L_out > 1 else 1,
                               o_stride_n=out.stride(2))
        f = TecmSarForecast(w=w, coef=coef.data_ptr(), d=self.d, D=self.D, s=self.s, n_ar=len(self.ar_lags),
                            n_ma=len(self.ma_lags), ar_lags=_lag_array(self.ar_lags), ma_lags=_lag_array(self.ma_lags))
        check(lib().tecm_sar_forecast(C.byref(f), stream_ptr()), "tecm_sar_forecast")
        return out

    def forecast_windows(self, dataset, indices: Sequence[int], channel: int = 0) -> torch.Tensor:
        """Forecasts for the windows `indices` of a `SlidingWindowSamplerDataset` as a (B, L_out, N, 1) device tensor, the
        layout of the model's output: one launch for any number of windows.  Reads `channel` of the feature-scaled X as
        it is, like the other baselines of `tecmollm.evaluate`.  The model must have been fitted on every node."""
        idx = [int(i) for i in indices]
        for i in idx:
            if not 0 <= i < dataset.num_samples:
                raise IndexError(f"Index {i} is out of bounds for a dataset of size {dataset.num_samples}")
        T, H, W, Cc = dataset.X.shape
        starts = [dataset.sample_indices[i] for i in idx]
        out = self.forecast_series(dataset.X.view(T, H * W, Cc), starts, dataset.L_in, dataset.L_out, channel)
        return out.unsqueeze(-1)

    def predict(self, node_indices, steps: int) -> dict:
        """{node: (steps,) float64} for the fitted nodes among `node_indices`: the forecast from the end of the training
        series, whose last min(T, 1024) steps are the window."""
        if self.coef_ is None:
            raise ValueError("SarimaBaseline.predict() before fit()")
        tail = torch.as_tensor(self.tail_).to(self.device).unsqueeze(-1).contiguous()
        out = self.forecast_series(tail, [0], tail.shape[0], int(steps)).cpu().numpy().astype(np.float64)
        col = {int(n): j for j, n in enumerate(self.nodes_)}
        return {int(n): out[0, :, col[int(n)]] for n in node_indices if int(n) in col}


# ------------------------------------------------------------------------------------ LinearBaseline
LINEAR_DEFAULT_LAGS = 48


def linear_pairs(lags, channel: int, exog, L_in: int):
    """The (channel, look-back) predictor pairs of a `LinearBaseline`: `lags` of `channel` (None: 1 .. min(L_in, 48)), then
    the `exog` pairs.  Look-back 1 is the last input step.  Raises ValueError for what no descriptor can hold; the library
    checks the rest against the data (`tecm_lin_gram_supported`)."""
    lags = range(1, min(int(L_in), LINEAR_DEFAULT_LAGS) + 1) if lags is None else lags
    try:
        pairs = [(int(channel), int(l)) for l in lags] + [(int(c), int(l)) for c, l in exog]
    except (TypeError, ValueError):
        raise ValueError(f"lags must be integers and exog (channel, lag) pairs, got {lags!r} and {exog!r}")
    if len(pairs) + 1 > _lib.TECM_LIN_MAX_P:
        raise ValueError(f"{len(pairs)} predictors and the intercept exceed {_lib.TECM_LIN_MAX_P}")
    if len(set(pairs)) != len(pairs):
        raise ValueError(f"a predictor pair is given twice in {pairs}")
    for c, l in pairs:
        if c < 0 or not 1 <= l <= _lib.TECM_LIN_MAX_LAG:
            raise ValueError(f"pair {(c, l)}: channels must not be negative and look-backs lie in [1, {_lib.TECM_LIN_MAX_LAG}]")
    return pairs


def _pair_arrays(pairs):
    chan, lag = (C.c_int32 * 64)(), (C.c_int32 * 64)()
    for p, (c, l) in enumerate(pairs, start=1):
        chan[p], lag[p] = c, l
    return chan, lag


def _gram_desc(pairs, T, N, Cc, Ty, L_in, H, first, step, count, pooled=False) -> TecmLinGram:
    chan, lag = _pair_arrays(pairs)
    return TecmLinGram(T=int(T), Ty=int(Ty), N=int(N), C=int(Cc), P=len(pairs) + 1, H=int(H), L_in=int(L_in), pooled=int(bool(pooled)),
                       chan=chan, lag=lag, first=int(first), step=int(step), count=int(count))


def linear_gram_geometry(pairs, T, N, Cc, Ty, L_in, H, first, step, count):
    """(nodes per block, windows per staged chunk) of the `tecm_lin_gram` launch for this shape, asked of the library (pure
    host arithmetic: no GPU needed); ValueError with the library's reason when the shape is not served."""
    tile, chunk = C.c_int32(), C.c_int32()
    desc = _gram_desc(pairs, T, N, Cc, Ty, L_in, H, first, step, count)
    if not lib().tecm_lin_gram_supported(C.byref(desc), C.byref(tile), C.byref(chunk)):
        raise ValueError(lib().tecm_last_error().decode("utf-8", "replace"))
    return tile.value, chunk.value


def linear_gram(X: torch.Tensor, ys: torch.Tensor, pairs, L_in: int, H: int, first: int, step: int, count: int, pooled: bool = False):
    """The normal equations of every window a = first + i step, i < count: X (T, N, C) contiguous float32 and ys (Ty, N)
    float32 of any non-negative strides, both on the device -> (gram (N, P, P+H) float64 = [G | R], gram_pooled (P, P+H) or
    None).  One running fp64 sum per entry in ascending window order: the bits of a sequential host loop."""
    require_gpu_tensor(X, "X")
    require_gpu_tensor(ys, "ys")
    if X.dim() != 3 or not X.is_contiguous():
        raise ValueError(f"X must be a contiguous (T, N, C) tensor, got {tuple(X.shape)}")
    T, N, Cc = X.shape
    if ys.dim() != 2 or ys.shape[1] != N:
        raise ValueError(f"ys must be (Ty, {N}), got {tuple(ys.shape)}")
    desc = _gram_desc(pairs, T, N, Cc, ys.shape[0], L_in, H, first, step, count, pooled)
    if not lib().tecm_lin_gram_supported(C.byref(desc), None, None):
        raise ValueError(lib().tecm_last_error().decode("utf-8", "replace"))
    P = len(pairs) + 1
    gram = torch.empty(N, P, P + int(H), device=X.device, dtype=torch.float64)
    gp = torch.empty(P, P + int(H), device=X.device, dtype=torch.float64) if pooled else None
    desc.X, desc.ys, desc.ys_stride_t, desc.ys_stride_n = X.data_ptr(), ys.data_ptr(), ys.stride(0), ys.stride(1)
    desc.gram, desc.gram_pooled = gram.data_ptr(), None if gp is None else gp.data_ptr()
    check(lib().tecm_lin_gram(C.byref(desc), stream_ptr()), "tecm_lin_gram")
    return gram, gp


def linear_solve(gram: torch.Tensor, alpha: float):
    """gram (N, P, P+H) float64 on the device -> (coef (N, P, H), coef_t (P, H, N), status (N) int32): the ridge solutions of
    (G + alpha diag(0, 1, ..., 1)) W = R by Cholesky, `coef_t` the node-fastest copy the forecast reads."""
    require_gpu_tensor(gram, "gram", torch.float64)
    if gram.dim() != 3 or gram.shape[2] <= gram.shape[1] or not gram.is_contiguous():
        raise ValueError(f"gram must be a contiguous (N, P, P + H) tensor, got {tuple(gram.shape)}")
    N, P, H = gram.shape[0], gram.shape[1], gram.shape[2] - gram.shape[1]
    coef = torch.empty(N, P, H, device=gram.device, dtype=torch.float64)
    coef_t = torch.empty(P, H, N, device=gram.device, dtype=torch.float64)
    status = torch.empty(N, device=gram.device, dtype=torch.int32)
    s = TecmLinSolve(gram=gram.data_ptr(), N=N, P=P, H=H, alpha=float(alpha), coef=coef.data_ptr(), coef_t=coef_t.data_ptr(),
                     status=status.data_ptr())
    check(lib().tecm_lin_solve(C.byref(s), stream_ptr()), "tecm_lin_solve")
    return coef, coef_t, status


def rebuilt_target_series(Y: torch.Tensor) -> torch.Tensor:
    """The target-scaled series behind a materialised Y (T, N, L_out), `Y[i, :, h] = Ys[i + 1 + h]`: (T + L_out, N) whose
    rows 1 .. T are `Y[:, :, 0]` and whose last L_out - 1 rows are the last row's remaining horizons, in one
    concatenation.  Row 0 is not in Y (no window's target reaches it) and is NaN."""
    head = torch.full_like(Y[:1, :, 0], float("nan"))
    return torch.cat([head, Y[:, :, 0], Y[-1, :, 1:].t()])


def _progression(indices, num_samples: int):
    """(first, step, count) of `indices` among a dataset's samples: None is every sample; else a range or a sequence that is
    one (ascending, constant difference)."""
    if indices is None:
        idx = range(num_samples)
    else:
        try:
            idx = indices if isinstance(indices, range) else [int(i) for i in indices]
        except (TypeError, ValueError):
            raise ValueError(f"indices must be None or a range-like arithmetic progression, got {indices!r}")
    if len(idx) == 0:
        raise ValueError("fit() needs at least one window")
    first, step = int(idx[0]), int(idx[1]) - int(idx[0]) if len(idx) > 1 else 1
    if step < 1 or any(int(idx[i]) != first + i * step for i in range(len(idx))):
        raise ValueError("indices must be None or a range-like arithmetic progression with a positive step")
    if first < 0 or first + (len(idx) - 1) * step >= num_samples:
        raise ValueError(f"indices leave the dataset's {num_samples} samples")
    return first, step, len(idx)


class LinearBaseline:
    """A per-node (or, with `pooled`, one shared) ridge regression from the input window to the L_out targets, fitted on
    the device against the target-scaled series (see the module docstring).  Predictors: the intercept, `lags` of
    `channel` (None: the last min(L_in, 48) steps), then the `exog` (channel, lag) pairs; look-back 1 is the last input
    step.  After `fit`, numpy only: `coef_` (N or 1, P, H) float64 with row 0 the intercept, `status_` (N or 1) int32 with
    the bits `DEGENERATE` (a Cholesky pivot vanished: the intercept-only model, whose forecast is the mean training target)
    and `NONFINITE` (a NaN / inf in the node's data: NaN coefficients), `pairs_` and `n_windows_`."""
    DEGENERATE, NONFINITE = _lib.TECM_LIN_DEGENERATE, _lib.TECM_LIN_NONFINITE

    def __init__(self, lags=None, channel: int = 0, exog=(), alpha: float = 1.0, pooled: bool = False,
                 device: Union[str, torch.device] = "cuda"):
        if not float(alpha) >= 0.0:
            raise ValueError(f"alpha must not be negative, got {alpha!r}")
        self.lags = None if lags is None else list(lags)
        self.channel, self.exog = int(channel), list(exog)
        linear_pairs(self.lags, self.channel, self.exog, LINEAR_DEFAULT_LAGS)          # refuse bad pairs now
        self.alpha, self.pooled, self.device = float(alpha), bool(pooled), torch.device(device)
        self.coef_ = self.status_ = self.pairs_ = self.n_windows_ = self.L_in_ = self.H_ = self.num_nodes_ = self.tail_ = None
        self._coef_dev = None

    # joblib / pickle: numpy only
    def __getstate__(self):
        state = {k: v for k, v in self.__dict__.items() if k != "_coef_dev"}
        state["device"] = str(self.device)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.device, self._coef_dev = torch.device(state["device"]), None

    def fit_series(self, X: torch.Tensor, ys: torch.Tensor, L_in: int, L_out: int, first: int, step: int,
                   count: int) -> "LinearBaseline":
        """Fits on the windows a = first + i step, i < count, of X (T, N, C) and the target-scaled series ys (Ty, N), device
        tensors both: inputs X[a : a + L_in], targets ys[a + L_in : a + L_in + L_out]."""
        pairs = linear_pairs(self.lags, self.channel, self.exog, L_in)
        log.info("Fitting the linear baseline (%d predictors, %d windows)...", len(pairs), count)
        gram, gp = linear_gram(X, ys, pairs, L_in, L_out, first, step, count, self.pooled)
        coef, coef_t, status = linear_solve(gp.unsqueeze(0) if self.pooled else gram, self.alpha)
        self._coef_dev = coef_t.view(coef_t.shape[0], coef_t.shape[1]) if self.pooled else coef_t
        self.coef_, self.status_ = coef.cpu().numpy(), status.cpu().numpy()
        self.pairs_, self.n_windows_, self.L_in_, self.H_, self.num_nodes_ = pairs, int(count), int(L_in), int(L_out), X.shape[1]
        self.tail_ = X[X.shape[0] - int(L_in):].cpu().numpy()
        log.info("Linear baseline fitted: %d degenerate, %d non-finite.", int((self.status_ & 1 != 0).sum()),
                 int((self.status_ & 2 != 0).sum()))
        return self

    def fit(self, dataset, indices=None) -> "LinearBaseline":
        """Fits on every sample of a `SlidingWindowSamplerDataset` or `SeriesWindowDataset`, or on the samples `indices`:
        a range, or a sequence that is an ascending arithmetic progression (anything else raises ValueError)."""
        first, step, count = _progression(indices, dataset.num_samples)
        T, Hh, W, Cc = dataset.X.shape
        N = Hh * W
        if "Ys" in dataset.__dict__:
            ys = dataset.Ys.view(dataset.Ys.shape[0], N)
        else:
            ys = rebuilt_target_series(dataset.Y.view(dataset.Y.shape[0], N, dataset.Y.shape[3]))
        return self.fit_series(dataset.X.view(T, N, Cc), ys, dataset.L_in, dataset.L_out, first * dataset.stride,
                               step * dataset.stride, count)

    def _coef_on(self, device) -> torch.Tensor:
        if self.coef_ is None:
            raise ValueError("LinearBaseline used before fit()")
        if self._coef_dev is None or self._coef_dev.device != device:
            c = torch.as_tensor(self.coef_)
            self._coef_dev = (c[0] if self.pooled else c.permute(1, 2, 0)).contiguous().to(device)
        return self._coef_dev

    def forecast_series(self, X: torch.Tensor, starts: Sequence[int], L_in: int, L_out: int, out: torch.Tensor = None,
                        coef: torch.Tensor = None, host_check: bool = True) -> torch.Tensor:
        """Forecasts from the windows X[a : a + L_in], a in `starts`, of a (T, N, C) float32 device tensor: (B, L_out, N)
        float32, or written into `out` (any strides).  `coef` on the device, float64, (P, H, N) node-fastest or (P, H) for
        every node, replaces the fitted coefficients.  Without `host_check` a window outside [0, T - L_in] reaches the
        kernel, which writes NaN."""
        require_gpu_tensor(X, "X")
        if X.dim() != 3 or not X.is_contiguous():
            raise ValueError(f"X must be a contiguous (T, N, C) tensor, got {tuple(X.shape)}")
        T, N, Cc = X.shape
        if self.pairs_ is None:
            raise ValueError("LinearBaseline used before fit()")
        if int(L_out) != self.H_:
            raise ValueError(f"fitted for {self.H_} horizons, asked for L_out = {L_out}")
        P = len(self.pairs_) + 1
        coef = self._coef_on(X.device) if coef is None else coef
        require_gpu_tensor(coef, "coef", torch.float64)
        if tuple(coef.shape) not in ((P, self.H_, N), (P, self.H_)) or not coef.is_contiguous():
            raise ValueError(f"coefficients of shape {tuple(coef.shape)} do not fit {P} predictors x {self.H_} horizons x {N} nodes")
        host = torch.tensor([int(a) for a in starts], dtype=torch.int64)
        B = host.numel()
        if B == 0:
            raise ValueError("forecast_series() needs at least one window")
        if out is None:
            out = torch.empty(B, int(L_out), N, device=X.device, dtype=torch.float32)
        require_gpu_tensor(out, "out")
        if out.shape != (B, int(L_out), N):
            raise ValueError(f"out must be {(B, int(L_out), N)}, got {tuple(out.shape)}")
        dev_starts = host.to(X.device, non_blocking=True)
        w = TecmWindowBaseline(X=X.data_ptr(), starts=dev_starts.data_ptr(), starts_host_check=host.data_ptr() if host_check else None,
                               T=T, N=N, C=Cc, channel=0, L_in=int(L_in), L_out=int(L_out), B=B, mode=0, period=0,
                               out=out.data_ptr(), o_stride_b=out.stride(0), o_stride_h=out.stride(1) if L_out > 1 else 1,
                               o_stride_n=out.stride(2))
        chan, lag = _pair_arrays(self.pairs_)
        f = TecmLinForecast(w=w, coef=coef.data_ptr(), coef_stride_n=1 if coef.dim() == 3 else 0, P=P, chan=chan, lag=lag)
        check(lib().tecm_lin_forecast(C.byref(f), stream_ptr()), "tecm_lin_forecast")
        return out

    def forecast_windows(self, dataset, indices: Sequence[int]) -> torch.Tensor:
        """Forecasts for the windows `indices` of a dataset as a (B, L_out, N, 1) device tensor, the layout of the model's
        output: one launch for any number of windows.  The dataset's L_out must equal the fitted one."""
        if self.coef_ is None:
            raise ValueError("LinearBaseline used before fit()")
        if dataset.L_out != self.H_:
            raise ValueError(f"fitted for {self.H_} horizons, the dataset has L_out = {dataset.L_out}")
        idx = [int(i) for i in indices]
        for i in idx:
            if not 0 <= i < dataset.num_samples:
                raise IndexError(f"Index {i} is out of bounds for a dataset of size {dataset.num_samples}")
        T, Hh, W, Cc = dataset.X.shape
        starts = [dataset.sample_indices[i] for i in idx]
        return self.forecast_series(dataset.X.view(T, Hh * W, Cc), starts, dataset.L_in, dataset.L_out).unsqueeze(-1)

    def predict(self, node_indices, steps: int) -> dict:
        """{node: (steps,) float64}, steps <= the fitted L_out, for the nodes among `node_indices`: the forecast from the
        end of the series the model was fitted on, whose last L_in rows are the window."""
        if self.coef_ is None:
            raise ValueError("LinearBaseline.predict() before fit()")
        if not 1 <= int(steps) <= self.H_:
            raise ValueError(f"fitted for {self.H_} horizons, asked for {steps} steps")
        tail = torch.as_tensor(self.tail_).to(self.device).contiguous()
        out = self.forecast_series(tail, [0], self.L_in_, self.H_).cpu().numpy().astype(np.float64)
        return {int(n): out[0, :int(steps), int(n)] for n in node_indices if 0 <= int(n) < self.num_nodes_}


# ------------------------------------------------------------------------------------ AnalogBaseline
ANALOG_DEFAULT_MATCH = LINEAR_DEFAULT_LAGS
ANALOG_NO_KEY = -1           # the key of an archive row that admits no query (no time feature, no condition, a negative id)


def analog_limits(k, match_len, L_in, L_out=1):
    """Checks K, m and L_out against what the kernels serve and returns (K, m): `match_len` None is min(L_in, 48).
    ValueError naming the argument otherwise."""
    k = int(k)
    if not 1 <= k <= _lib.TECM_ANALOG_MAX_K:
        raise ValueError(f"k must lie in [1, {_lib.TECM_ANALOG_MAX_K}], got {k}")
    L_in = int(L_in)
    m = min(L_in, ANALOG_DEFAULT_MATCH) if match_len is None else int(match_len)
    if not 1 <= m <= min(L_in, _lib.TECM_ANALOG_MAX_M):
        raise ValueError(f"match_len must lie in [1, min(L_in, {_lib.TECM_ANALOG_MAX_M})] (L_in = {L_in}), got {m}")
    if not 1 <= int(L_out) <= _lib.TECM_ANALOG_MAX_H:
        raise ValueError(f"L_out must lie in [1, {_lib.TECM_ANALOG_MAX_H}], got {L_out}")
    return k, m


def _search_desc(Ta, Ty, Tq, N, Cc, channel, L_in, L_out, m, K, S, exclude=0, Tk=0, origin_shift=0) -> TecmAnalogSearch:
    return TecmAnalogSearch(Ta=int(Ta), Ty=int(Ty), Tq=int(Tq), N=int(N), C=int(Cc), channel=int(channel), L_in=int(L_in),
                            L_out=int(L_out), m=int(m), K=int(K), S=int(S), exclude=int(exclude), Tk=int(Tk),
                            origin_shift=int(origin_shift))


def analog_search_geometry(Ta, Ty, Tq, N, Cc, channel, L_in, L_out, m, K, S):
    """(candidates per staged chunk, queries per block, valid candidates) of the `tecm_analog_search` launch for this shape,
    asked of the library (pure host arithmetic: no GPU needed); ValueError with the library's reason when it is not served."""
    chunk, tile, ncand = C.c_int32(), C.c_int32(), C.c_int64()
    desc = _search_desc(Ta, Ty, Tq, N, Cc, channel, L_in, L_out, m, K, S)
    if not lib().tecm_analog_search_supported(C.byref(desc), C.byref(chunk), C.byref(tile), C.byref(ncand)):
        raise ValueError(lib().tecm_last_error().decode("utf-8", "replace"))
    return chunk.value, tile.value, ncand.value


def _require_device(t, name: str, dtype, shape=None, contiguous=True) -> None:
    """ValueError naming `name` unless `t` is a device tensor of `dtype` (and `shape`, and contiguous)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on the GPU; the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def analog_search(A: torch.Tensor, Ty: int, Xq: torch.Tensor, starts: Sequence[int], L_in: int, L_out: int, m: int, K: int,
                  channel: int = 0, key_arch: torch.Tensor = None, key_q: torch.Tensor = None, exclude: int = 0,
                  origin_shift: int = 0, host_check: bool = True):
    """The K nearest archive segments of every (window, node): A (N, Ta) node-major and Xq (Tq, N, C), contiguous float32
    device tensors; `starts` the windows' first rows in Xq; `Ty` the rows of the outcome series (it bounds the
    candidates).  `key_arch` (Tk) and `key_q` (S) int32 device tensors admit only candidates whose origin row carries
    the query's key; `exclude` > 0 refuses candidates whose origin lies nearer than that to the query's, which is
    `start + L_in + origin_shift` in archive rows.  Returns (idx (S, N, K) int32, dist (S, N, K) float32, count (S, N)
    int32) on the device: ascending by (dist, idx), unused places -1 / +inf."""
    _require_device(A, "archive", torch.float32)
    _require_device(Xq, "X", torch.float32)
    if A.dim() != 2:
        raise ValueError(f"archive must be (N, Ta) node-major, got {tuple(A.shape)}")
    if Xq.dim() != 3:
        raise ValueError(f"X must be (T, N, C), got {tuple(Xq.shape)}")
    N, Ta = A.shape
    Tq, Nq, Cc = Xq.shape
    if Nq != N:
        raise ValueError(f"num_nodes: the archive holds {N} nodes, the query dataset {Nq}")
    host = torch.tensor([int(a) for a in starts], dtype=torch.int64)
    S = host.numel()
    if S == 0:
        raise ValueError("analog_search() needs at least one window")
    if (key_arch is None) != (key_q is None):
        raise ValueError("key_arch and key_q must be given together")
    Tk = 0
    if key_arch is not None:
        _require_device(key_arch, "key_arch", torch.int32)
        _require_device(key_q, "key_q", torch.int32, (S,))
        Tk = key_arch.numel()
    desc = _search_desc(Ta, Ty, Tq, N, Cc, channel, L_in, L_out, m, K, S, exclude, Tk, origin_shift)
    if key_arch is not None:
        desc.key_arch, desc.key_q = key_arch.data_ptr(), key_q.data_ptr()
    if not lib().tecm_analog_search_supported(C.byref(desc), None, None, None):
        raise ValueError(lib().tecm_last_error().decode("utf-8", "replace"))
    idx = torch.empty(S, N, int(K), device=A.device, dtype=torch.int32)
    dist = torch.empty(S, N, int(K), device=A.device, dtype=torch.float32)
    count = torch.empty(S, N, device=A.device, dtype=torch.int32)
    dev_starts = host.to(A.device, non_blocking=True)
    desc.A, desc.Xq, desc.starts = A.data_ptr(), Xq.data_ptr(), dev_starts.data_ptr()
    desc.starts_host_check = host.data_ptr() if host_check else None
    desc.idx, desc.dist, desc.count = idx.data_ptr(), dist.data_ptr(), count.data_ptr()
    check(lib().tecm_analog_search(C.byref(desc), stream_ptr()), "tecm_analog_search")
    return idx, dist, count


def analog_forecast(Y: torch.Tensor, idx: torch.Tensor, count: torch.Tensor, m: int, L_out: int, out: torch.Tensor = None,
                    want_mean: bool = True, want_members: bool = False):
    """From the outcomes Y (N, Ty) node-major and a search result: (mean (B, L_out, N) float32 or None, members (K, B, L_out,
    N) float32 or None).  `out` (B, L_out, N), any strides, receives the mean in place."""
    _require_device(Y, "outcomes", torch.float32)
    _require_device(idx, "idx", torch.int32)
    if Y.dim() != 2 or idx.dim() != 3 or idx.shape[1] != Y.shape[0]:
        raise ValueError(f"outcomes must be (N, Ty) and idx (B, N, K), got {tuple(Y.shape)} and {tuple(idx.shape)}")
    B, N, K = idx.shape
    _require_device(count, "count", torch.int32, (B, N))
    L_out = int(L_out)
    if out is None and want_mean:
        out = torch.empty(B, L_out, N, device=Y.device, dtype=torch.float32)
    if out is not None:
        _require_device(out, "out", torch.float32, (B, L_out, N), contiguous=False)
    members = torch.empty(K, B, L_out, N, device=Y.device, dtype=torch.float32) if want_members else None
    f = TecmAnalogForecast(Y=Y.data_ptr(), Ty=Y.shape[1], idx=idx.data_ptr(), count=count.data_ptr(), N=N, K=K, m=int(m),
                           L_out=L_out, B=B, out=None if out is None else out.data_ptr(),
                           o_stride_b=0 if out is None else out.stride(0),
                           o_stride_h=0 if out is None else (out.stride(1) if L_out > 1 else 1),
                           o_stride_n=0 if out is None else out.stride(2), members=None if members is None else members.data_ptr())
    check(lib().tecm_analog_forecast(C.byref(f), stream_ptr()), "tecm_analog_forecast")
    return out, members


class AnalogBaseline:
    """The analog ensemble (AnEn): for every (window, node) the `k` stretches of the training record that lie nearest, in
    squared distance over the last `match_len` input steps of `channel` (None: min(L_in, 48)), to the window's own, and
    what followed them -- `k` members whose plain mean is the point forecast.  Non-parametric: `fit` only stores the record.

    Admission.  `same_slot` (default) admits only stretches whose forecast origin falls in the query's time-of-day slot
    (`time_features[origin, 0]`); `condition=` of `fit` and of the query methods adds a group id, e.g. the storm level of
    `window_groups_by_index`: an int32 id per row of the dataset's X, or per sample of the dataset (mapped to the sample's
    origin row; the other rows then admit nothing).  A negative id admits nothing.  An archive row without a time feature
    (the row just past X when the target series is longer) admits nothing while keys are in use.  When the query dataset
    is the object the baseline was fitted on, stretches whose origin lies nearer than `exclude` rows to the query's are
    refused (None: match_len + L_out, so that neither segment nor outcome overlaps the query's targets).

    What it is not: one channel only, matched per node (no whole-map analog date), uniform weights, and the outcomes are
    taken as they are (no adjustment of their level to the query's).

    After `fit`: `n_candidates_`, `match_len_`, `H_` (the dataset's L_out), `num_nodes_`, `row0_` (the first dataset row
    of the archive).  The archive and its outcomes live on the device node-major, 2 * N * Ta * 4 bytes together (408 MB at
    N = 2911 and Ta = 17 520, four years of 2-hour maps); pickling copies them to numpy (`archive_`,
    `outcomes_`) and the device tensors are rebuilt on first use."""

    _DEVICE_STATE = ("_A_dev", "_Y_dev", "_keys_dev", "_fit_ref")

    def __init__(self, k: int = 16, match_len=None, channel: int = 0, same_slot: bool = True, exclude=None,
                 device: Union[str, torch.device] = "cuda"):
        analog_limits(k, match_len, _lib.TECM_ANALOG_MAX_M if match_len is None else max(int(match_len), 1))
        if int(channel) < 0:
            raise ValueError(f"channel must not be negative, got {channel}")
        if exclude is not None and int(exclude) < 0:
            raise ValueError(f"exclude must not be negative, got {exclude}")
        self.k, self.match_len, self.channel = int(k), None if match_len is None else int(match_len), int(channel)
        self.same_slot, self.exclude, self.device = bool(same_slot), None if exclude is None else int(exclude), torch.device(device)
        self.n_candidates_ = self.match_len_ = self.H_ = self.num_nodes_ = self.row0_ = self.L_in_ = None
        self.archive_ = self.outcomes_ = self.slot_ = self.cond_ = None
        self._A_dev = self._Y_dev = self._keys_dev = self._fit_ref = None

    # joblib / pickle: numpy only
    def __getstate__(self):
        state = {k: v for k, v in self.__dict__.items() if k not in self._DEVICE_STATE}
        if self._A_dev is not None and self.archive_ is None:
            state["archive_"], state["outcomes_"] = self._A_dev.cpu().numpy(), self._Y_dev.cpu().numpy()
        state["device"] = str(self.device)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.device = torch.device(state["device"])
        self._A_dev = self._Y_dev = self._keys_dev = self._fit_ref = None

    # ---- keys
    @staticmethod
    def _condition_rows(condition, dataset, rows: int):
        """`condition` -> an int32 numpy id per row 0 .. rows - 1 of the dataset's series (ANALOG_NO_KEY where none is given)."""
        cond = condition.cpu().numpy() if isinstance(condition, torch.Tensor) else np.asarray(condition)
        if cond.ndim != 1 or not np.issubdtype(cond.dtype, np.integer):
            raise ValueError("condition must be a 1-D integer array")
        origins = np.asarray(dataset.sample_indices, dtype=np.int64) + dataset.L_in
        out = np.full(max(rows, int(origins.max()) + 1 if origins.size else 0), ANALOG_NO_KEY, dtype=np.int64)
        if cond.shape[0] == dataset.X.shape[0]:
            out[:cond.shape[0]] = cond[:out.shape[0]]
        elif cond.shape[0] == dataset.num_samples:
            out[origins] = cond
        else:
            raise ValueError(f"condition must hold one id per row of X ({dataset.X.shape[0]}) or per sample ({dataset.num_samples}), "
                             f"got {cond.shape[0]}")
        out[out < 0] = ANALOG_NO_KEY
        return out[:rows].astype(np.int32)

    @staticmethod
    def _slot_rows(dataset, rows: int):
        tf = dataset.time_features[:, 0].to(torch.int32).cpu().numpy()
        out = np.full(rows, ANALOG_NO_KEY, dtype=np.int32)
        out[:min(rows, tf.shape[0])] = tf[:rows]
        return out

    @staticmethod
    def _combine(slot, cond):
        """key = cond * 12 + slot; ANALOG_NO_KEY where either is; None when neither rule is in use."""
        if slot is None and cond is None:
            return None
        if cond is None:
            return slot
        if slot is None:
            return cond
        key = cond.astype(np.int64) * SLOTS_PER_DAY + slot
        key[(slot < 0) | (cond < 0)] = ANALOG_NO_KEY
        return key.astype(np.int32)

    def fit(self, dataset, indices=None, condition=None) -> "AnalogBaseline":
        """Stores the record behind every sample of a `SlidingWindowSamplerDataset` or `SeriesWindowDataset`, or behind the
        samples `indices` (a range-like progression; the archive is the stretch of rows from the first sample's first
        input to the last sample's last target)."""
        first, step, count = _progression(indices, dataset.num_samples)
        T, Hh, W, Cc = dataset.X.shape
        N = Hh * W
        if not 0 <= self.channel < Cc:
            raise ValueError(f"channel {self.channel} lies outside [0, {Cc})")
        K, m = analog_limits(self.k, self.match_len, dataset.L_in, dataset.L_out)
        if "Ys" in dataset.__dict__:
            ys = dataset.Ys.view(dataset.Ys.shape[0], N)
        else:
            ys = rebuilt_target_series(dataset.Y.view(dataset.Y.shape[0], N, dataset.Y.shape[3]))
        row0 = dataset.sample_indices[first]
        last = dataset.sample_indices[first + (count - 1) * step]
        Ta, Ty = min(last + dataset.L_in, T) - row0, min(last + dataset.L_in + dataset.L_out, ys.shape[0]) - row0
        log.info("Storing the analog archive (%d rows, %d nodes)...", Ta, N)
        self._A_dev = dataset.X.view(T, N, Cc)[row0:row0 + Ta, :, self.channel].t().contiguous()
        self._Y_dev = ys[row0:row0 + Ty].t().contiguous()
        self.archive_ = self.outcomes_ = None
        self.slot_ = self._slot_rows(dataset, row0 + Ta + 1)[row0:] if self.same_slot else None
        self.cond_ = None if condition is None else self._condition_rows(condition, dataset, row0 + Ta + 1)[row0:]
        self._keys_dev = None
        _, _, ncand = analog_search_geometry(Ta, Ty, dataset.L_in, N, 1, 0, dataset.L_in, dataset.L_out, m, K, 1)
        self.n_candidates_, self.match_len_, self.H_, self.num_nodes_, self.row0_, self.L_in_ = int(ncand), m, dataset.L_out, N, int(row0), dataset.L_in
        self._fit_ref = weakref.ref(dataset)
        return self

    def _require_fitted(self):
        if self.n_candidates_ is None:
            raise ValueError("AnalogBaseline used before fit()")

    def _archive_on(self, device):
        self._require_fitted()
        if self._A_dev is None or self._A_dev.device != device:
            if self.archive_ is None:
                self.archive_, self.outcomes_ = self._A_dev.cpu().numpy(), self._Y_dev.cpu().numpy()
            self._A_dev = torch.as_tensor(self.archive_).to(device).contiguous()
            self._Y_dev = torch.as_tensor(self.outcomes_).to(device).contiguous()
            self._keys_dev = None
        return self._A_dev, self._Y_dev

    def _keys_on(self, device, slot=True):
        key = self._combine(self.slot_ if slot else None, self.cond_)
        if key is None:
            return None
        if self._keys_dev is None or self._keys_dev.device != device:
            self._keys_dev = torch.as_tensor(key).to(device)
        return self._keys_dev

    def _query_keys(self, dataset, idx, condition):
        """The int32 key of every query window on the device (the slot column is read there: no host synchronisation), or
        None when no rule is in use.  A window without a valid key gets -2, which no archive row carries."""
        if self.cond_ is not None and condition is None:
            raise ValueError("condition: the baseline was fitted with a condition, the query needs one too")
        if self.cond_ is None and condition is not None:
            raise ValueError("condition: the baseline was fitted without a condition")
        if not self.same_slot and condition is None:
            return None
        origins = np.asarray([dataset.sample_indices[i] for i in idx], dtype=np.int64) + dataset.L_in
        dev = dataset.X.device
        key = torch.zeros(len(idx), device=dev, dtype=torch.int32)
        if self.same_slot:
            key = dataset.time_features[torch.as_tensor(origins).to(dev, non_blocking=True), 0].to(torch.int32)
        if condition is not None:
            cond = torch.as_tensor(self._condition_rows(condition, dataset, int(origins.max()) + 1)[origins]).to(dev, non_blocking=True)
            key = torch.where(cond < 0, -2, cond * (SLOTS_PER_DAY if self.same_slot else 1) + key).to(torch.int32)
        return key

    def search_windows(self, dataset, indices: Sequence[int], condition=None):
        """(idx (B, N, K) int32, dist (B, N, K) float32, count (B, N) int32) on the device for the windows `indices` of a
        dataset of the fitted node count and L_out: `idx` are archive rows (add `row0_` for rows of the fitted dataset)."""
        self._require_fitted()
        T, Hh, W, Cc = dataset.X.shape
        if Hh * W != self.num_nodes_:
            raise ValueError(f"num_nodes: fitted on {self.num_nodes_} nodes, the dataset has {Hh * W}")
        if dataset.L_out != self.H_:
            raise ValueError(f"L_out: fitted for {self.H_} horizons, the dataset has L_out = {dataset.L_out}")
        if dataset.L_in < self.match_len_:
            raise ValueError(f"match_len: the fitted match length {self.match_len_} exceeds the dataset's L_in = {dataset.L_in}")
        if not 0 <= self.channel < Cc:
            raise ValueError(f"channel {self.channel} lies outside [0, {Cc})")
        idx = [int(i) for i in indices]
        for i in idx:
            if not 0 <= i < dataset.num_samples:
                raise IndexError(f"Index {i} is out of bounds for a dataset of size {dataset.num_samples}")
        if not idx:
            raise ValueError("search_windows() needs at least one window")
        A, Y = self._archive_on(dataset.X.device)
        key_arch = self._keys_on(A.device)
        key_q = self._query_keys(dataset, idx, condition)
        own = self._fit_ref is not None and self._fit_ref() is dataset
        exclude = (self.match_len_ + self.H_ if self.exclude is None else self.exclude) if own else 0
        starts = [dataset.sample_indices[i] for i in idx]
        return analog_search(A, Y.shape[1], dataset.X.view(T, Hh * W, Cc), starts, dataset.L_in, dataset.L_out, self.match_len_,
                             self.k, self.channel, key_arch, key_q, exclude, -self.row0_)

    def _forecast(self, dataset, indices, condition, want_mean, want_members):
        idx, _, count = self.search_windows(dataset, indices, condition)
        return analog_forecast(self._Y_dev, idx, count, self.match_len_, self.H_, want_mean=want_mean, want_members=want_members) + (count,)

    def members(self, dataset, indices: Sequence[int], condition=None, reorder=None) -> torch.Tensor:
        """The K outcomes of every (window, node) as (K, B, L_out, N), the layout of `ensemble_members`: member k is what
        followed the k-th nearest stretch; NaN where fewer than k + 1 stretches were admitted.  `reorder` (a template of
        `tecmollm.coherence`): the members of every cell are handed to the member indices in the template's rank order, in
        place -- member k is then a map and no longer the k-th nearest; NaNs go to the template's highest ranks."""
        members = self._forecast(dataset, indices, condition, False, True)[1]
        if reorder is not None:
            reorder.apply_(members, dataset, indices)
        return members

    def forecast_windows(self, dataset, indices: Sequence[int], condition=None) -> torch.Tensor:
        """The mean of the members as a (B, L_out, N, 1) device tensor, the layout of the model's output; NaN where no
        stretch was admitted."""
        return self._forecast(dataset, indices, condition, True, False)[0].unsqueeze(-1)

    def predict(self, node_indices, steps: int) -> dict:
        """{node: (steps,) float64}, steps <= the fitted L_out, for the nodes among `node_indices`: the forecast from the end
        of the archive, whose last match_len rows are the query; the exclusion keeps it from finding itself.  With
        `same_slot` the query's slot is the one after the archive's last row; a fitted condition is not applied."""
        self._require_fitted()
        if not 1 <= int(steps) <= self.H_:
            raise ValueError(f"fitted for {self.H_} horizons, asked for {steps} steps")
        A, Y = self._archive_on(self.device if self._A_dev is None else self._A_dev.device)
        m, Ta = self.match_len_, A.shape[1]
        tail = A[:, Ta - m:].t().contiguous().unsqueeze(-1)                 # (m, N, 1)
        key_arch = key_q = None
        if self.same_slot:
            key_arch = torch.as_tensor(self.slot_).to(A.device)
            key_q = torch.tensor([(int(self.slot_[Ta - 1]) + 1) % SLOTS_PER_DAY], dtype=torch.int32).to(A.device)
        exclude = m + self.H_ if self.exclude is None else self.exclude
        idx, _, count = analog_search(A, Y.shape[1], tail, [0], m, self.H_, m, self.k, 0, key_arch, key_q, exclude, Ta - m)
        out = analog_forecast(Y, idx, count, m, self.H_)[0].cpu().numpy().astype(np.float64)
        return {int(n): out[0, :int(steps), int(n)] for n in node_indices if 0 <= int(n) < self.num_nodes_}


def save_baseline(model, path):
    import joblib
    joblib.dump(model, path)
    log.info("Baseline model saved to %s", path)


def load_baseline(path):
    import joblib
    log.info("Loading baseline model from %s", path)
    return joblib.load(path)
