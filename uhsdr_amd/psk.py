"""Batched BPSK decoder, varicode to text (uhsdr_psk_*, include/uhsdr.h): one decoder per channel,
fed 12 ksps audio sample by sample; exact to the firmware's Psk_Demodulator_ProcessSample."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .rtty import RttyOutputs

SPEED_31, SPEED_63, SPEED_125 = range(3)


class PskOutputs(RttyOutputs):
    """The decoder's outputs (text ring, totals, symbol) as host arrays, and the bytes new since the
    last read.  `device`: the pointers are device memory (copied out), else host memory."""

    def __init__(self, lib, channels: int, capacity: int, device: bool, text: int, total: int, symbol: int):
        super().__init__(lib, channels, capacity, device, text, total)
        self.symbol_ptr = symbol

    def read_symbol(self):
        """symbol float32 [C], rx_last_symbol: the averaged phase at the last bit decision"""
        return self._get(self.symbol_ptr, np.empty(self.channels, np.float32))


class PskDecoder:
    def __init__(self, channels: int, speed: int = SPEED_31, capacity: int = 64, host: bool = False, stream: int | None = None):
        self.lib = _abi.load()
        self.channels, self.host, self.text_capacity = int(channels), bool(host), int(capacity)
        args = (self.channels, int(speed), self.text_capacity)
        h = C.c_void_p()
        if host:
            _abi.check(self.lib.uhsdr_psk_create_host(*args, C.byref(h)), "uhsdr_psk_create_host")
        else:
            _abi.check(self.lib.uhsdr_psk_create(*args, C.c_void_p(stream or 0), C.byref(h)), "uhsdr_psk_create")
        self.handle = h
        p = [C.c_void_p() for _ in range(3)]
        _abi.check(self.lib.uhsdr_psk_outputs(h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2])), "uhsdr_psk_outputs")
        self.outputs = PskOutputs(self.lib, self.channels, self.text_capacity, not host, *(x.value for x in p))

    def reset(self) -> None:
        _abi.check(self.lib.uhsdr_psk_reset(self.handle), "uhsdr_psk_reset")
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
            _abi.check(self.lib.uhsdr_psk_process_host(self.handle, samples.ctypes.data_as(C.c_void_p), n, stride),
                       "uhsdr_psk_process_host")
        else:
            if not samples.is_floating_point() or samples.element_size() != 4 or not samples.is_contiguous():
                raise ValueError("samples must be a contiguous float32 tensor")
            _abi.check(self.lib.uhsdr_psk_process(self.handle, C.c_void_p(samples.data_ptr()), n, stride),
                       "uhsdr_psk_process")

    def synchronize(self) -> None:
        _abi.check(self.lib.uhsdr_psk_synchronize(self.handle), "uhsdr_psk_synchronize")

    def read(self):
        """(text uint8 [C][capacity] ring, total uint32 [C]) after everything enqueued"""
        self.synchronize()
        return self.outputs.read()

    def symbol(self):
        self.synchronize()
        return self.outputs.read_symbol()

    def new_text(self):
        self.synchronize()
        return self.outputs.new_text()

    def close(self) -> None:
        if self.handle:
            self.lib.uhsdr_psk_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
