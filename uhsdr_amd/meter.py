"""Batched signal meter (uhsdr_meter_*, include/uhsdr.h): per channel and display frame the dBm and
dBm/Hz readout, the S-units and the SNAP carrier estimate of the firmware's front panel, from frames
of sd.FFT_MagData; exact to UiSpectrum_CalculateDBm, RadioManagement_HandleIqGainAndSMeter and
UiDriver_HandleSMeter.  The meter inside the spectrum kernel is Spectrum.set_meter."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._handle import Handle

# the rows of uhsdr_meter_io in its order, with their element types
OUTPUTS = (("dbm_cur", np.float32), ("dbmhz_cur", np.float32), ("dbm", np.float32), ("dbmhz", np.float32),
           ("s_count", np.int32), ("snap_carrier_freq", np.uint32))


def meter_config(**overrides) -> _abi.MeterConfig:
    """uhsdr_meter_config_default with fields replaced"""
    cfg = _abi.MeterConfig()
    _abi.load().uhsdr_meter_config_default(C.byref(cfg))
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


def meter_plan(cfg: _abi.MeterConfig) -> _abi.MeterPlan:
    plan = _abi.MeterPlan()
    _abi.check(_abi.load().uhsdr_meter_plan_build(C.byref(cfg), C.byref(plan)), "uhsdr_meter_plan_build")
    return plan


class Meter(Handle):
    kind = "meter"

    def __init__(self, channels: int, cfg: _abi.MeterConfig | None = None, host: bool = False, stream: int | None = None):
        self.cfg = cfg if cfg is not None else meter_config()
        self._create(channels, (C.byref(self.cfg),), host, stream)
        self.plan = meter_plan(self.cfg)
        self.fft_len = self.plan.fft_len

    def io(self, frames: int, cw_signal=None, **rows) -> _abi.MeterIo:
        """uhsdr_meter_io from rows [C][frames] named as OUTPUTS (numpy arrays for a host meter,
        torch cuda tensors for a device one) and the optional uint8 input cw_signal"""
        io = _abi.MeterIo()
        types = dict(OUTPUTS, cw_signal=np.uint8)
        for name, x in dict(rows, cw_signal=cw_signal).items():
            if x is None:
                continue
            if name not in types:
                raise ValueError(f"no row named {name}")
            if tuple(x.shape) != (self.channels, frames) or not self._fits(x, types[name]):
                raise ValueError(f"{name} must be a contiguous {np.dtype(types[name]).name} [{self.channels}][{frames}]")
            setattr(io, name, self._ptr(x).value)
        return io

    def _run(self, call: str, mag, cw_signal, rows) -> None:
        if len(mag.shape) != 3 or mag.shape[0] != self.channels or mag.shape[2] != self.fft_len or not self._fits(mag, np.float32):
            raise ValueError(f"mag must be a contiguous float32 [{self.channels}][frames][{self.fft_len}]")
        frames = int(mag.shape[1])
        io = self.io(frames, cw_signal, **rows)
        self._call(call, self._ptr(mag), frames, C.byref(io))

    def process_mag(self, mag, cw_signal=None, **rows) -> None:
        """mag: float32 [C][frames][fft_len] cuda tensor, frames of FFT_MagData in natural bin order;
        rows: tensors [C][frames] named as OUTPUTS, written per frame (stream-ordered)"""
        if self.host:
            raise ValueError("a host meter runs process_mag_host")
        self._run("process_mag", mag, cw_signal, rows)

    def process_mag_host(self, mag: np.ndarray, cw_signal: np.ndarray | None = None) -> dict:
        """the same on numpy arrays by a host meter; returns the six rows by name"""
        if not self.host:
            raise ValueError("a device meter runs process_mag")
        rows = {name: np.empty((self.channels, mag.shape[1]), dt) for name, dt in OUTPUTS}
        self._run("process_mag_host", mag, cw_signal, rows)
        return rows

    def state(self) -> dict:
        """the last outputs per channel, [C] each by name, after everything enqueued"""
        out = {name: np.empty(self.channels, dt) for name, dt in OUTPUTS}
        self._call("state", *(out[name].ctypes.data_as(C.c_void_p) for name, _ in OUTPUTS))
        return out
