"""Batched RTTY decoder, Baudot to text (uhsdr_rtty_*, include/uhsdr.h): one decoder per channel,
fed 12 ksps audio sample by sample; exact to the firmware's Rtty_Demodulator_ProcessSample."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi

SHIFT_85, SHIFT_170, SHIFT_200, SHIFT_425, SHIFT_450, SHIFT_850 = range(6)
SPEED_45, SPEED_50 = range(2)
STOP_1, STOP_1_5, STOP_2 = range(3)


class RttyOutputs:
    """The decoder's outputs (text ring, totals) as host arrays, and the bytes new since the last
    read.  `device`: the pointers are device memory (copied out), else host memory."""

    def __init__(self, lib, channels: int, capacity: int, device: bool, text: int, total: int):
        self.lib, self.channels, self.capacity, self.device = lib, channels, capacity, device
        self.ptr = (text, total)
        self.seen = np.zeros(channels, np.uint32)

    def _get(self, ptr, arr):
        if self.device:
            _abi.check(self.lib.uhsdr_copy_to_host(arr.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), arr.nbytes), "uhsdr_copy_to_host")
        else:
            C.memmove(arr.ctypes.data, ptr, arr.nbytes)
        return arr

    def read(self):
        """(text uint8 [C][capacity] ring, total uint32 [C]); the work enqueued must be complete."""
        return (self._get(self.ptr[0], np.empty((self.channels, self.capacity), np.uint8)),
                self._get(self.ptr[1], np.empty(self.channels, np.uint32)))

    def new_text(self):
        """Per channel, the bytes emitted since the last call (the last `capacity` of them if more)."""
        text, total = self.read()
        out = []
        for c in range(self.channels):
            first = max(int(self.seen[c]), int(total[c]) - self.capacity)
            out.append(bytes(text[c, np.arange(first, int(total[c])) % self.capacity]))
        self.seen = total.copy()
        return out


class RttyDecoder:
    def __init__(self, channels: int, shift: int = SHIFT_170, speed: int = SPEED_45, stopbits: int = STOP_1_5,
                 atc_disable: bool = False, capacity: int = 64, host: bool = False, stream: int | None = None):
        self.lib = _abi.load()
        self.channels, self.host, self.text_capacity = int(channels), bool(host), int(capacity)
        args = (self.channels, int(shift), int(speed), int(stopbits), int(bool(atc_disable)), self.text_capacity)
        h = C.c_void_p()
        if host:
            _abi.check(self.lib.uhsdr_rtty_create_host(*args, C.byref(h)), "uhsdr_rtty_create_host")
        else:
            _abi.check(self.lib.uhsdr_rtty_create(*args, C.c_void_p(stream or 0), C.byref(h)), "uhsdr_rtty_create")
        self.handle = h
        p = [C.c_void_p() for _ in range(2)]
        _abi.check(self.lib.uhsdr_rtty_outputs(h, C.byref(p[0]), C.byref(p[1])), "uhsdr_rtty_outputs")
        self.outputs = RttyOutputs(self.lib, self.channels, self.text_capacity, not host, *(x.value for x in p))

    def reset(self) -> None:
        _abi.check(self.lib.uhsdr_rtty_reset(self.handle), "uhsdr_rtty_reset")
        self.outputs.seen[:] = 0

    def process(self, samples, n: int | None = None) -> None:
        """samples: float32 [C][stride], 12 ksps audio: a contiguous numpy array for a host decoder, a
        torch cuda tensor for a device one (stream-ordered).  Decodes the first `n` (default: all)
        of every row."""
        if len(samples.shape) != 2 or samples.shape[0] != self.channels:
            raise ValueError("samples must be [C][stride]")
        stride = int(samples.shape[1])
        n = stride if n is None else int(n)
        if self.host:
            if samples.dtype != np.float32 or not samples.flags.c_contiguous:
                raise ValueError("samples must be a contiguous float32 array")
            _abi.check(self.lib.uhsdr_rtty_process_host(self.handle, samples.ctypes.data_as(C.c_void_p), n, stride),
                       "uhsdr_rtty_process_host")
        else:
            if not samples.is_floating_point() or samples.element_size() != 4 or not samples.is_contiguous():
                raise ValueError("samples must be a contiguous float32 tensor")
            _abi.check(self.lib.uhsdr_rtty_process(self.handle, C.c_void_p(samples.data_ptr()), n, stride),
                       "uhsdr_rtty_process")

    def synchronize(self) -> None:
        _abi.check(self.lib.uhsdr_rtty_synchronize(self.handle), "uhsdr_rtty_synchronize")

    def read(self):
        self.synchronize()
        return self.outputs.read()

    def new_text(self):
        self.synchronize()
        return self.outputs.new_text()

    def close(self) -> None:
        if self.handle:
            self.lib.uhsdr_rtty_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
