"""Batched spectral noise reduction (uhsdr_nr_*, include/uhsdr.h): one instance per channel, fed
128-sample frames at 6 or 12 ksps (process_frames) or the 12 ksps stream around them (process); exact
to the firmware's spectral_noise_reduction_3 and AudioDriver_RxProcessorNoiseReduction."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi

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


class NrProcessor:
    def __init__(self, channels: int, cfg: _abi.NrConfig | None = None, host: bool = False, stream: int | None = None):
        self.lib = _abi.load()
        self.channels, self.host = int(channels), bool(host)
        self.cfg = cfg if cfg is not None else nr_config()
        h = C.c_void_p()
        if host:
            _abi.check(self.lib.uhsdr_nr_create_host(self.channels, C.byref(self.cfg), C.byref(h)), "uhsdr_nr_create_host")
        else:
            _abi.check(self.lib.uhsdr_nr_create(self.channels, C.byref(self.cfg), C.c_void_p(stream or 0), C.byref(h)), "uhsdr_nr_create")
        self.handle = h

    def reset(self) -> None:
        _abi.check(self.lib.uhsdr_nr_reset(self.handle), "uhsdr_nr_reset")

    def _rows(self, x, out):
        if len(x.shape) != 2 or x.shape[0] != self.channels or tuple(out.shape) != tuple(x.shape):
            raise ValueError("in and out must be [C][stride]")
        if self.host:
            for a in (x, out):
                if a.dtype != np.float32 or not a.flags.c_contiguous:
                    raise ValueError("rows must be contiguous float32 arrays")
            return x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), int(x.shape[1])
        for a in (x, out):
            if not a.is_floating_point() or a.element_size() != 4 or not a.is_contiguous():
                raise ValueError("rows must be contiguous float32 tensors")
        return C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), int(x.shape[1])

    def process_frames(self, x, out, frames: int | None = None) -> None:
        """x, out: float32 [C][stride], numpy arrays for a host processor, torch cuda tensors for a
        device one (stream-ordered); runs the first `frames` (default: all whole) frames of every row."""
        pi, po, stride = self._rows(x, out)
        frames = stride // FRAME if frames is None else int(frames)
        fn = self.lib.uhsdr_nr_process_frames_host if self.host else self.lib.uhsdr_nr_process_frames
        _abi.check(fn(self.handle, pi, po, frames, stride), "uhsdr_nr_process_frames")

    def process(self, x, out, n: int | None = None) -> None:
        """The 12 ksps stream: the first `n` (default: all; a multiple of 8) samples of every row."""
        pi, po, stride = self._rows(x, out)
        n = stride if n is None else int(n)
        fn = self.lib.uhsdr_nr_process_host if self.host else self.lib.uhsdr_nr_process
        _abi.check(fn(self.handle, pi, po, n, stride), "uhsdr_nr_process")

    def synchronize(self) -> None:
        _abi.check(self.lib.uhsdr_nr_synchronize(self.handle), "uhsdr_nr_synchronize")

    def state(self):
        """(first_time int32 [C], NN int32 [C], power_ratio float32 [C]) after everything enqueued"""
        ft, nn = np.empty(self.channels, np.int32), np.empty(self.channels, np.int32)
        pr = np.empty(self.channels, np.float32)
        _abi.check(self.lib.uhsdr_nr_state(self.handle, ft.ctypes.data_as(C.c_void_p), nn.ctypes.data_as(C.c_void_p),
                                           pr.ctypes.data_as(C.c_void_p)), "uhsdr_nr_state")
        return ft, nn, pr

    def close(self) -> None:
        if self.handle:
            self.lib.uhsdr_nr_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
