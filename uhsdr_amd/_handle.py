"""What the Python handles of the per-channel modules (cwdec, rtty, psk, digimod, cwgen, nr) share:
the copy-out of an output, the text ring's reader, and the life of a handle."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi


def fetch(lib, ptr: int, shape, dtype, device: bool) -> np.ndarray:
    """An output as a host array: copied from device memory, or from the host memory of a host handle."""
    arr = np.empty(shape, dtype)
    if arr.nbytes == 0:
        return arr
    if device:
        _abi.check(lib.uhsdr_copy_to_host(arr.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), arr.nbytes), "uhsdr_copy_to_host")
    else:
        C.memmove(arr.ctypes.data, ptr, arr.nbytes)
    return arr


class TextRing:
    """A decoder's outputs as host arrays (text ring, totals and further per-channel values), and the
    bytes new since the last read.  `device`: the pointers are device memory (copied out), else
    host memory.  `extra`: (pointer, dtype) of every [C] output that read() returns after the two."""

    def __init__(self, lib, channels: int, capacity: int, device: bool, text: int, total: int, extra=()):
        self.lib, self.channels, self.capacity, self.device = lib, channels, capacity, device
        self.ptr = (text, total) + tuple(p for p, _ in extra)
        self._extra = tuple(extra)
        self.seen = np.zeros(channels, np.uint32)

    def _get(self, ptr, shape, dtype):
        return fetch(self.lib, ptr, shape, dtype, self.device)

    def read(self):
        """(text uint8 [C][capacity] ring, total uint32 [C], the extra outputs); the work enqueued must be complete."""
        return (self._get(self.ptr[0], (self.channels, self.capacity), np.uint8), self._get(self.ptr[1], self.channels, np.uint32),
                *(self._get(p, self.channels, d) for p, d in self._extra))

    def new_text(self):
        """Per channel, the bytes emitted since the last call (the last `capacity` of them if more)."""
        text, total = self.read()[:2]
        out = []
        for c in range(self.channels):
            first = max(int(self.seen[c]), int(total[c]) - self.capacity)
            out.append(bytes(text[c, np.arange(first, int(total[c])) % self.capacity]))
        self.seen = total.copy()
        return out


class Handle:
    """A handle of the C ABI; `kind` is the infix of its calls (uhsdr_<kind>_create, ...)."""
    kind = ""
    handle = None

    def _create(self, channels: int, args: tuple, host: bool, stream: int | None) -> None:
        self.lib = _abi.load()
        self.channels, self.host = int(channels), bool(host)
        h = C.c_void_p()
        if host:
            self._call("create_host", self.channels, *args, C.byref(h), handle=False)
        else:
            self._call("create", self.channels, *args, C.c_void_p(stream or 0), C.byref(h), handle=False)
        self.handle = h

    def _call(self, name: str, *args, handle: bool = True):
        fn = f"uhsdr_{self.kind}_{name}"
        _abi.check(getattr(self.lib, fn)(*((self.handle,) if handle else ()), *args), fn)

    def _pointers(self, name: str, count: int) -> list:
        """the `count` pointers a call like uhsdr_<kind>_outputs hands out"""
        p = [C.c_void_p() for _ in range(count)]
        self._call(name, *(C.byref(x) for x in p))
        return [x.value for x in p]

    def _fits(self, x, dtype) -> bool:
        """x is what a row argument must be: a contiguous numpy array of `dtype` for a host handle,
        a contiguous torch tensor of it for a device handle"""
        dt = np.dtype(dtype)
        if self.host:
            return x.dtype == dt and x.flags.c_contiguous
        return x.is_floating_point() == (dt.kind == "f") and x.element_size() == dt.itemsize and x.is_contiguous()

    def _ptr(self, x) -> C.c_void_p:
        return x.ctypes.data_as(C.c_void_p) if self.host else C.c_void_p(x.data_ptr())

    def rows(self, x, dtype, name: str):
        """(pointer, stride) of x, which must be [C][stride] of dtype"""
        if len(x.shape) != 2 or x.shape[0] != self.channels:
            raise ValueError(f"{name} must be [C][stride]")
        if not self._fits(x, dtype):
            raise ValueError(f"{name} must be a contiguous {np.dtype(dtype).name} {'array' if self.host else 'tensor'}")
        return self._ptr(x), int(x.shape[1])

    def _process(self, x, dtype, name: str, n: int | None) -> None:
        """the one-row process call: the first `n` (default: all) of every row of x"""
        p, stride = self.rows(x, dtype, name)
        self._call("process_host" if self.host else "process", p, stride if n is None else int(n), stride)

    def reset(self) -> None:
        self._call("reset")

    def set_stream(self, stream: int) -> None:
        self._call("set_stream", C.c_void_p(stream))

    def synchronize(self) -> None:
        self._call("synchronize")

    def close(self) -> None:
        if self.handle:
            getattr(self.lib, f"uhsdr_{self.kind}_destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TextSender(Handle):
    """A modulator or generator with a text queue per channel."""

    def put_text(self, text) -> np.ndarray:
        """text: one bytes object per channel (or one for all).  Appends what fits to every channel's
        queue and returns the accepted counts, int32 [C].  Waits for the work enqueued."""
        if isinstance(text, (bytes, bytearray)):
            text = [bytes(text)] * self.channels
        if len(text) != self.channels:
            raise ValueError("one text per channel")
        length = np.array([len(t) for t in text], np.int32)
        stride = max(1, int(length.max()))
        rows = np.zeros((self.channels, stride), np.uint8)
        for c, t in enumerate(text):
            rows[c, :len(t)] = np.frombuffer(bytes(t), np.uint8)
        accepted = np.zeros(self.channels, np.int32)
        self._call("put_text", rows.ctypes.data_as(C.c_void_p), length.ctypes.data_as(C.c_void_p), stride,
                   accepted.ctypes.data_as(C.c_void_p))
        return accepted

    def _fetch(self, ptr, shape, dtype) -> np.ndarray:
        return fetch(self.lib, ptr, shape, dtype, not self.host)


class TextDecoder(Handle):
    """A decoder with a TextRing in `outputs`."""

    def reset(self) -> None:
        super().reset()
        self.outputs.seen[:] = 0

    def read(self):
        """the outputs' read() after everything enqueued"""
        self.synchronize()
        return self.outputs.read()

    def new_text(self):
        self.synchronize()
        return self.outputs.new_text()
