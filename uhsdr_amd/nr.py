"""Batched spectral noise reduction (uhsdr_nr_*, include/uhsdr.h): one instance per channel, fed
128-sample frames at 6 or 12 ksps (process_frames) or the 12 ksps stream around them (process); exact
to the firmware's spectral_noise_reduction_3 and AudioDriver_RxProcessorNoiseReduction."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._handle import Handle

FRAME = 128          # samples per frame
BLOCK = 8            # the stream's granularity: the firmware's block of 32 codec frames at 12 ksps


def nr_config(**overrides) -> _abi.NrConfig:
    """uhsdr_nr_config_default with fields replaced; `nr_strength` sets alpha as the firmware does."""
    lib = _abi.load()
    cfg = _abi.NrConfig()
    lib.uhsdr_nr_config_default(C.byref(cfg))
    for k, v in overrides.items():
        if k == "nr_strength":
            cfg.alpha = lib.uhsdr_nr_alpha_from_strength(int(v))
        else:
            setattr(cfg, k, v)
    return cfg


def nr_band(cfg: _abi.NrConfig):
    """(VAD_low, VAD_high) of a configuration; raises where uhsdr_nr_create would refuse it"""
    lo, hi = C.c_int32(), C.c_int32()
    _abi.check(_abi.load().uhsdr_nr_band(C.byref(cfg), C.byref(lo), C.byref(hi)), "uhsdr_nr_band")
    return lo.value, hi.value


class NrProcessor(Handle):
    kind = "nr"

    def __init__(self, channels: int, cfg: _abi.NrConfig | None = None, host: bool = False, stream: int | None = None):
        self.cfg = cfg if cfg is not None else nr_config()
        self._create(channels, (C.byref(self.cfg),), host, stream)

    def _rows(self, x, out):
        if len(x.shape) != 2 or x.shape[0] != self.channels or tuple(out.shape) != tuple(x.shape):
            raise ValueError("in and out must be [C][stride]")
        if not (self._fits(x, np.float32) and self._fits(out, np.float32)):
            raise ValueError("rows must be contiguous float32 " + ("arrays" if self.host else "tensors"))
        return self._ptr(x), self._ptr(out), int(x.shape[1])

    def process_frames(self, x, out, frames: int | None = None) -> None:
        """x, out: float32 [C][stride], numpy arrays for a host processor, torch cuda tensors for a
        device one (stream-ordered); runs the first `frames` (default: all whole) frames of every row."""
        pi, po, stride = self._rows(x, out)
        self._call("process_frames_host" if self.host else "process_frames", pi, po, stride // FRAME if frames is None else int(frames), stride)

    def process(self, x, out, n: int | None = None) -> None:
        """The 12 ksps stream: the first `n` (default: all; a multiple of 8) samples of every row."""
        pi, po, stride = self._rows(x, out)
        self._call("process_host" if self.host else "process", pi, po, stride if n is None else int(n), stride)

    def state(self):
        """(first_time int32 [C], NN int32 [C], power_ratio float32 [C]) after everything enqueued"""
        ft, nn = np.empty(self.channels, np.int32), np.empty(self.channels, np.int32)
        pr = np.empty(self.channels, np.float32)
        self._call("state", ft.ctypes.data_as(C.c_void_p), nn.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p))
        return ft, nn, pr
