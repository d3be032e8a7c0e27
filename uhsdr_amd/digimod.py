"""Batched RTTY and BPSK modulators, text to 48 ksps int16 audio (uhsdr_rttymod_*, uhsdr_pskmod_*,
include/uhsdr.h): one modulator and one text queue per channel; exact to the firmware's
Rtty_Modulator_GenSample and Psk_Modulator_GenSample."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .rtty import SHIFT_170, SPEED_45, STOP_1_5
from .psk import SPEED_31

NO_TXOFF = 0xFFFFFFFF
PSK_OFF, PSK_PREAMBLE, PSK_ACTIVE, PSK_POSTAMBLE, PSK_INACTIVE = range(5)
EOT = b"\x04"


class _Modulator:
    """What the two have in common; `kind` is the infix of the C calls."""
    kind = ""

    def _create(self, channels: int, args: tuple, capacity: int, host: bool, stream: int | None) -> None:
        self.lib = _abi.load()
        self.channels, self.host, self.text_capacity = int(channels), bool(host), int(capacity)
        h = C.c_void_p()
        if host:
            self._call("create_host", self.channels, *args, self.text_capacity, C.byref(h), handle=False)
        else:
            self._call("create", self.channels, *args, self.text_capacity, C.c_void_p(stream or 0), C.byref(h), handle=False)
        self.handle = h
        p = [C.c_void_p() for _ in range(3)]
        self._call("outputs", C.byref(p[0]), C.byref(p[1]), C.byref(p[2]))
        self._out = [x.value for x in p]

    def _call(self, name: str, *args, handle: bool = True):
        fn = f"uhsdr_{self.kind}_{name}"
        _abi.check(getattr(self.lib, fn)(*((self.handle,) if handle else ()), *args), fn)

    def reset(self) -> None:
        self._call("reset")

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

    def process(self, audio, n: int | None = None) -> None:
        """audio: int16 [C][stride]: a contiguous numpy array for a host modulator, a torch cuda tensor
        for a device one (stream-ordered).  Writes the next `n` (default: all) samples of every row."""
        if len(audio.shape) != 2 or audio.shape[0] != self.channels:
            raise ValueError("audio must be [C][stride]")
        stride = int(audio.shape[1])
        n = stride if n is None else int(n)
        if self.host:
            if audio.dtype != np.int16 or not audio.flags.c_contiguous:
                raise ValueError("audio must be a contiguous int16 array")
            self._call("process_host", audio.ctypes.data_as(C.c_void_p), n, stride)
        else:
            if audio.is_floating_point() or audio.element_size() != 2 or not audio.is_contiguous():
                raise ValueError("audio must be a contiguous int16 tensor")
            self._call("process", C.c_void_p(audio.data_ptr()), n, stride)

    def generate(self, n: int) -> np.ndarray:
        """the next n samples of every channel as a host array int16 [C][n]"""
        if self.host:
            audio = np.zeros((self.channels, n), np.int16)
            self.process(audio)
            return audio
        import torch
        audio = torch.zeros((self.channels, n), dtype=torch.int16, device="cuda")
        self.process(audio)
        self.synchronize()
        return audio.cpu().numpy()

    def set_stream(self, stream: int) -> None:
        self._call("set_stream", C.c_void_p(stream))

    def synchronize(self) -> None:
        self._call("synchronize")

    def _get(self, k: int, dtype):
        self.synchronize()
        arr = np.empty(self.channels, dtype)
        if self.host:
            C.memmove(arr.ctypes.data, self._out[k], arr.nbytes)
        else:
            _abi.check(self.lib.uhsdr_copy_to_host(arr.ctypes.data_as(C.c_void_p), C.c_void_p(self._out[k]), arr.nbytes), "uhsdr_copy_to_host")
        return arr

    def consumed(self) -> np.ndarray:
        """uint32 [C], characters taken from the queue since reset"""
        return self._get(0, np.uint32)

    def txoff_at(self) -> np.ndarray:
        """uint32 [C], the first sample since reset that requested TX-off, NO_TXOFF if none"""
        return self._get(1, np.uint32)

    def state(self) -> np.ndarray:
        """uint8 [C], the BPSK modulator state (PSK_OFF .. PSK_INACTIVE); 0 for RTTY"""
        return self._get(2, np.uint8)

    def close(self) -> None:
        if getattr(self, "handle", None):
            getattr(self.lib, f"uhsdr_{self.kind}_destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RttyModulator(_Modulator):
    kind = "rttymod"

    def __init__(self, channels: int, shift: int = SHIFT_170, speed: int = SPEED_45, stopbits: int = STOP_1_5,
                 capacity: int = 128, host: bool = False, stream: int | None = None):
        self._create(channels, (int(shift), int(speed), int(stopbits)), capacity, host, stream)

    def start_tx(self) -> None:
        """Rtty_Modulator_StartTX on every channel"""
        self._call("start_tx")


class PskModulator(_Modulator):
    kind = "pskmod"

    def __init__(self, channels: int, speed: int = SPEED_31, capacity: int = 128, host: bool = False, stream: int | None = None):
        self._create(channels, (int(speed),), capacity, host, stream)

    def prepare_tx(self) -> None:
        """Psk_Modulator_PrepareTx on every channel"""
        self._call("prepare_tx")
