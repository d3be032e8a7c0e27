"""Batched CW decoder back end, Morse to text (uhsdr_cwdec_*, include/uhsdr.h): one decoder per
channel, fed the mark/space byte of every CW block; exact to the firmware's CW_Decode."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi

SPIKECANCEL_OFF, SPIKECANCEL_SPIKE, SPIKECANCEL_SHORT = 0, 1, 2


class TextOutputs:
    """The decoder's outputs (text ring, totals, wpm) as host arrays, and the bytes new since the
    last read.  `device`: the pointers are device memory (copied out), else host memory."""

    def __init__(self, lib, channels: int, capacity: int, device: bool, text: int, total: int, wpm: int):
        self.lib, self.channels, self.capacity, self.device = lib, channels, capacity, device
        self.ptr = (text, total, wpm)
        self.seen = np.zeros(channels, np.uint32)

    def _get(self, ptr, arr):
        if self.device:
            _abi.check(self.lib.uhsdr_copy_to_host(arr.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), arr.nbytes), "uhsdr_copy_to_host")
        else:
            C.memmove(arr.ctypes.data, ptr, arr.nbytes)
        return arr

    def read(self):
        """(text uint8 [C][capacity] ring, total uint32 [C], wpm uint8 [C]); the work enqueued must be complete."""
        return (self._get(self.ptr[0], np.empty((self.channels, self.capacity), np.uint8)),
                self._get(self.ptr[1], np.empty(self.channels, np.uint32)),
                self._get(self.ptr[2], np.empty(self.channels, np.uint8)))

    def new_text(self):
        """Per channel, the bytes emitted since the last call (the last `capacity` of them if more)."""
        text, total, _ = self.read()
        out = []
        for c in range(self.channels):
            first = max(int(self.seen[c]), int(total[c]) - self.capacity)
            out.append(bytes(text[c, np.arange(first, int(total[c])) % self.capacity]))
        self.seen = total.copy()
        return out


class CwDecoder:
    def __init__(self, channels: int, blocksize: int = 88, spikecancel: int = SPIKECANCEL_OFF, text_capacity: int = 64,
                 host: bool = False, stream: int | None = None):
        self.lib = _abi.load()
        self.channels, self.blocksize, self.host = int(channels), int(blocksize), bool(host)
        self.text_capacity = int(text_capacity)
        h = C.c_void_p()
        if host:
            _abi.check(self.lib.uhsdr_cwdec_create_host(self.channels, self.blocksize, int(spikecancel), self.text_capacity,
                                                        C.byref(h)), "uhsdr_cwdec_create_host")
        else:
            _abi.check(self.lib.uhsdr_cwdec_create(self.channels, self.blocksize, int(spikecancel), self.text_capacity,
                                                   C.c_void_p(stream or 0), C.byref(h)), "uhsdr_cwdec_create")
        self.handle = h
        p = [C.c_void_p() for _ in range(3)]
        _abi.check(self.lib.uhsdr_cwdec_outputs(h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2])), "uhsdr_cwdec_outputs")
        self.outputs = TextOutputs(self.lib, self.channels, self.text_capacity, not host, *(x.value for x in p))

    def reset(self) -> None:
        _abi.check(self.lib.uhsdr_cwdec_reset(self.handle), "uhsdr_cwdec_reset")
        self.outputs.seen[:] = 0

    def process(self, state, blocks: int | None = None) -> None:
        """state: uint8 [C][stride], one byte per CW block, non-zero = mark: a contiguous numpy array
        for a host decoder, a torch cuda tensor for a device one (stream-ordered).  Decodes the first
        `blocks` (default: all) of every row."""
        if len(state.shape) != 2 or state.shape[0] != self.channels:
            raise ValueError("state must be [C][stride]")
        stride = int(state.shape[1])
        blocks = stride if blocks is None else int(blocks)
        if self.host:
            if state.dtype != np.uint8 or not state.flags.c_contiguous:
                raise ValueError("state must be a contiguous uint8 array")
            _abi.check(self.lib.uhsdr_cwdec_process_host(self.handle, state.ctypes.data_as(C.c_void_p), blocks, stride),
                       "uhsdr_cwdec_process_host")
        else:
            if state.element_size() != 1 or not state.is_contiguous():
                raise ValueError("state must be a contiguous uint8 tensor")
            _abi.check(self.lib.uhsdr_cwdec_process(self.handle, C.c_void_p(state.data_ptr()), blocks, stride),
                       "uhsdr_cwdec_process")

    def synchronize(self) -> None:
        _abi.check(self.lib.uhsdr_cwdec_synchronize(self.handle), "uhsdr_cwdec_synchronize")

    def read(self):
        self.synchronize()
        return self.outputs.read()

    def new_text(self):
        self.synchronize()
        return self.outputs.new_text()

    def close(self) -> None:
        if self.handle:
            self.lib.uhsdr_cwdec_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def char_id(code: int) -> int:
    """CwGen_CharacterIdFunc: the character of a two-bits-per-element code (0xfe empty, 0xff unknown)."""
    return int(_abi.load().uhsdr_cwdec_char_id(int(code)))
