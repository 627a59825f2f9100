"""Device-side mirror of the reference's `src/models/baselines.py` (`HistoricalAverage`, `save_baseline`,
`load_baseline`).

`HistoricalAverage.fit` (:13-33) loops over nodes x 12 slots on the host with one masked `np.mean` each; here one
kernel (`tecm_slot_mean`) returns the (N, 12) table from a series that already lives on the device: fp64 sums in a fixed
order, so the table does not depend on the launch.  The series is read as float32, the dtype the processed splits
carry; a float64 input is rounded to it first.  `predict` (:35-45) is a row gather.

`SarimaBaseline` (:47-72) is NOT provided: it is a thin wrapper around statsmodels' SARIMAX, a host library this
project neither ships nor replaces.
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import Union

import numpy as np
import torch

from tecmollm._lib import TecmSlotMean, check, lib, require_gpu_tensor, stream_ptr

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


def save_baseline(model, path):
    import joblib
    joblib.dump(model, path)
    log.info("Baseline model saved to %s", path)


def load_baseline(path):
    import joblib
    log.info("Loading baseline model from %s", path)
    return joblib.load(path)
