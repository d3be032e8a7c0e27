"""Batched waterfall image (uhsdr_wfall_*, include/uhsdr.h): per channel the line ring of the
firmware's waterfall with its frequencies, and the panel's RGB565 rows of the last drawing of a call;
exact to UiSpectrum_DrawWaterfall behind the byte line (the ring, doubleLineStart and the vertical
step, the frequency-shift padding, the palette, the markers of
UiSpectrum_UpdateSpectrumPixelParameters).  The lines are the wfall row of the display stage."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._handle import Handle

# the outputs of uhsdr_wfall_io in its order, with their element types: [C][height][width] and [C][frames]
OUTPUTS = (("image", np.uint16), ("drawn", np.uint8))


def wfall_config(**overrides) -> _abi.WfallConfig:
    """uhsdr_wfall_config_default with fields replaced"""
    cfg = _abi.WfallConfig()
    _abi.load().uhsdr_wfall_config_default(C.byref(cfg))
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


def wfall_plan(cfg: _abi.WfallConfig) -> _abi.WfallPlan:
    plan = _abi.WfallPlan()
    _abi.check(_abi.load().uhsdr_wfall_plan_build(C.byref(cfg), C.byref(plan)), "uhsdr_wfall_plan_build")
    return plan


class Waterfall(Handle):
    kind = "wfall"

    def __init__(self, channels: int, cfg: _abi.WfallConfig | None = None, host: bool = False, stream: int | None = None):
        self.cfg = cfg if cfg is not None else wfall_config()
        self._create(channels, (C.byref(self.cfg),), host, stream)
        self.plan = wfall_plan(self.cfg)
        self.width, self.height = self.plan.width, self.plan.height

    def output_shape(self, name: str, frames: int) -> tuple:
        return (self.channels, self.height, self.width) if name == "image" else (self.channels, frames)

    def io(self, frames: int, **outputs) -> _abi.WfallIo:
        """uhsdr_wfall_io from outputs named as OUTPUTS (numpy arrays for a host handle, torch cuda
        tensors for a device one)"""
        io = _abi.WfallIo()
        types = dict(OUTPUTS)
        for name, x in outputs.items():
            if x is None:
                continue
            if name not in types:
                raise ValueError(f"no output named {name}")
            if tuple(x.shape) != self.output_shape(name, frames) or not self._fits(x, types[name]):
                raise ValueError(f"{name} must be a contiguous {np.dtype(types[name]).name} {self.output_shape(name, frames)}")
            setattr(io, name, self._ptr(x).value)
        return io

    def _run(self, call: str, lines, center_hz, outputs) -> None:
        if len(lines.shape) != 3 or lines.shape[0] != self.channels or lines.shape[2] != self.width or not self._fits(lines, np.uint8):
            raise ValueError(f"lines must be a contiguous uint8 [{self.channels}][frames][{self.width}]")
        frames = int(lines.shape[1])
        if center_hz is not None and (tuple(center_hz.shape) != (self.channels, frames) or not self._fits(center_hz, np.uint32)):
            raise ValueError(f"center_hz must be a contiguous 32-bit integer [{self.channels}][{frames}]")
        io = self.io(frames, **outputs)
        self._call(call, self._ptr(lines), self._ptr(center_hz) if center_hz is not None else None, frames, C.byref(io))

    def process_lines(self, lines, center_hz=None, image=None, drawn=None) -> None:
        """lines: uint8 [C][frames][width] cuda tensor, the wfall row of Display.process_avg; center_hz: int32
        tensor [C][frames] holding the uint32 bits of sd.FFT_frequency, or None (0); image, drawn: tensors as
        OUTPUTS or None; image is written only if a frame of the call draws (stream-ordered)"""
        if self.host:
            raise ValueError("a host waterfall runs process_lines_host")
        self._run("process_lines", lines, center_hz, dict(image=image, drawn=drawn))

    def process_lines_host(self, lines: np.ndarray, center_hz: np.ndarray | None = None, image: np.ndarray | None = None) -> dict:
        """the same on numpy arrays by a host handle; `image` (updated in place if a frame draws) or a
        new array of zeros; returns image and drawn by name"""
        if not self.host:
            raise ValueError("a device waterfall runs process_lines")
        out = dict(image=image if image is not None else np.zeros(self.output_shape("image", 0), np.uint16),
                   drawn=np.empty(self.output_shape("drawn", lines.shape[1]), np.uint8))
        self._run("process_lines_host", lines, center_hz, out)
        return out

    def state(self) -> dict:
        """sd.wfall_line, doubleLineStart and sd.wfall_line_update after everything enqueued"""
        v = [C.c_uint32() for _ in range(3)]
        self._call("state", *(C.byref(x) for x in v))
        return dict(zip(("wfall_line", "double_line_start", "wfall_line_update"), (int(x.value) for x in v)))
