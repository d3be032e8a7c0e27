"""Batched display stage (uhsdr_display_*, include/uhsdr.h): per channel and display frame the scope
trace heights and the waterfall line of palette indices of the firmware's panel, from frames of
sd.FFT_AVGData; exact to states 4 and 5 of UiSpectrum_RedrawSpectrum up to the LCD calls
(UiSpectrum_ScaleFFT, UiSpectrum_ScaleFFT2SpectrumWidth, the display's sliding AGC, the height of
UiSpectrum_DrawScope and the byte line of UiSpectrum_DrawWaterfall).  The stage inside the spectrum
kernel is Spectrum.set_display."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._handle import Handle

# the rows of uhsdr_display_io in its order, with their element types; the first two are
# [C][frames][width], the others [C][frames]
OUTPUTS = (("scope", np.uint16), ("wfall", np.uint8), ("offset", np.float32), ("min", np.float32))
WIDE = ("scope", "wfall")


def display_config(**overrides) -> _abi.DisplayConfig:
    """uhsdr_display_config_default with fields replaced"""
    cfg = _abi.DisplayConfig()
    _abi.load().uhsdr_display_config_default(C.byref(cfg))
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


def display_plan(cfg: _abi.DisplayConfig) -> _abi.DisplayPlan:
    plan = _abi.DisplayPlan()
    _abi.check(_abi.load().uhsdr_display_plan_build(C.byref(cfg), C.byref(plan)), "uhsdr_display_plan_build")
    return plan


class Display(Handle):
    kind = "display"

    def __init__(self, channels: int, cfg: _abi.DisplayConfig | None = None, host: bool = False, stream: int | None = None):
        self.cfg = cfg if cfg is not None else display_config()
        self._create(channels, (C.byref(self.cfg),), host, stream)
        self.plan = display_plan(self.cfg)
        self.fft_len, self.width = self.plan.fft_len, self.plan.width

    def row_shape(self, name: str, frames: int) -> tuple:
        return (self.channels, frames, self.width) if name in WIDE else (self.channels, frames)

    def io(self, frames: int, **rows) -> _abi.DisplayIo:
        """uhsdr_display_io from rows named as OUTPUTS (numpy arrays for a host display, torch cuda
        tensors for a device one)"""
        io = _abi.DisplayIo()
        types = dict(OUTPUTS)
        for name, x in rows.items():
            if x is None:
                continue
            if name not in types:
                raise ValueError(f"no row named {name}")
            if tuple(x.shape) != self.row_shape(name, frames) or not self._fits(x, types[name]):
                raise ValueError(f"{name} must be a contiguous {np.dtype(types[name]).name} {self.row_shape(name, frames)}")
            setattr(io, name, self._ptr(x).value)
        return io

    def _run(self, call: str, avg, edge, rows) -> None:
        if len(avg.shape) != 3 or avg.shape[0] != self.channels or avg.shape[2] != self.fft_len or not self._fits(avg, np.float32):
            raise ValueError(f"avg must be a contiguous float32 [{self.channels}][frames][{self.fft_len}]")
        frames = int(avg.shape[1])
        if edge is not None and (tuple(edge.shape) != (self.channels, frames) or not self._fits(edge, np.float32)):
            raise ValueError(f"edge must be a contiguous float32 [{self.channels}][{frames}]")
        io = self.io(frames, **rows)
        self._call(call, self._ptr(avg), self._ptr(edge) if edge is not None else None, frames, C.byref(io))

    def process_avg(self, avg, edge=None, **rows) -> None:
        """avg: float32 [C][frames][fft_len] cuda tensor, frames of FFT_AVGData in natural bin order;
        edge: float32 [C][frames] or None (0); rows: tensors named as OUTPUTS, written per frame
        (stream-ordered)"""
        if self.host:
            raise ValueError("a host display runs process_avg_host")
        self._run("process_avg", avg, edge, rows)

    def process_avg_host(self, avg: np.ndarray, edge: np.ndarray | None = None) -> dict:
        """the same on numpy arrays by a host display; returns the four rows by name"""
        if not self.host:
            raise ValueError("a device display runs process_avg")
        rows = {name: np.empty(self.row_shape(name, avg.shape[1]), dt) for name, dt in OUTPUTS}
        self._run("process_avg_host", avg, edge, rows)
        return rows

    def state(self) -> dict:
        """display_offset and the last min per channel, [C] each, after everything enqueued"""
        out = {name: np.empty(self.channels, np.float32) for name in ("offset", "min")}
        self._call("state", out["offset"].ctypes.data_as(C.c_void_p), out["min"].ctypes.data_as(C.c_void_p))
        return out
