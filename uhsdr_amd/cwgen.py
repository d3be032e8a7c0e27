"""Batched CW generator, key lines and text to 48 ksps I/Q (uhsdr_cwgen_*, include/uhsdr.h): one
keyer, one tone generator, one text queue and one echo ring per channel; exact to the firmware's
CwGen_Process."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._handle import TextSender

IAM_B, IAM_A, STRAIGHT, ULTIMATE = range(4)
DIT, DAH = 1, 2                                     # bits of a key byte
ACTIVE, TX_ON, TX_OFF = 1, 2, 4                     # bits of a flag byte
IDLE, DIT_CHECK, DAH_CHECK, KEY_DOWN, KEY_UP, PAUSE, WAIT = 0, 1, 3, 4, 5, 6, 7
BLOCK = 32
# rows of peek()
WORDS = ("port_state", "cw_state", "key_timer", "break_timer", "space_timer", "sm_tbl_ptr", "ultim", "cw_char", "sending_char", "acc", "keys")


class _Config(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("keyer_mode", "keyer_speed", "keyer_weight", "paddle_reverse", "rx_delay", "sidetone_freq")]


class CwGenerator(TextSender):
    kind = "cwgen"

    def __init__(self, channels: int, mode: int = IAM_B, speed: int = 20, weight: int = 100, reverse: bool = False, rx_delay: int = 8,
                 sidetone: int = 750, capacity: int = 128, echo_capacity: int = 256, host: bool = False, stream: int | None = None):
        self.text_capacity, self.echo_capacity = int(capacity), int(echo_capacity)
        cfg = _Config(int(mode), int(speed), int(weight), int(bool(reverse)), int(rx_delay), int(sidetone))
        self._create(channels, (C.byref(cfg), self.text_capacity, self.echo_capacity), host, stream)
        self._blocks = 0

    def set_speed(self, speed: int, weight: int = 100) -> None:
        """CwGen_SetSpeed; holds from the next process call on"""
        self._call("set_speed", int(speed), int(weight))

    def process(self, keys, i, q, n: int | None = None) -> None:
        """keys: uint8 [C][n/32]; i, q: float32 [C][stride].  Contiguous numpy arrays for a host
        generator, torch cuda tensors for a device one (stream-ordered).  Writes the next `n`
        (default: all) samples of every row."""
        if len(i.shape) != 2 or i.shape[0] != self.channels or tuple(q.shape) != tuple(i.shape):
            raise ValueError("i and q must be [C][stride]")
        stride = int(i.shape[1])
        n = stride if n is None else int(n)
        if tuple(keys.shape) != (self.channels, n // BLOCK):
            raise ValueError("keys must be [C][n/32]")
        if not (self._fits(keys, np.uint8) and self._fits(i, np.float32) and self._fits(q, np.float32)):
            raise ValueError("keys must be a contiguous uint8 array, i and q contiguous float32 arrays" if self.host else
                             "keys must be a contiguous uint8 tensor, i and q contiguous float32 tensors")
        self._call("process_host" if self.host else "process", self._ptr(keys), self._ptr(i), self._ptr(q), n, stride)
        self._blocks = n // BLOCK

    def generate(self, keys: np.ndarray):
        """keys uint8 [C][blocks] on the host -> (i, q) as host arrays float32 [C][32 * blocks]"""
        keys = np.ascontiguousarray(keys, np.uint8)
        n = BLOCK * keys.shape[1]
        if self.host:
            i, q = np.zeros((self.channels, n), np.float32), np.zeros((self.channels, n), np.float32)
            self.process(keys, i, q)
            return i, q
        import torch
        i = torch.zeros((self.channels, n), dtype=torch.float32, device="cuda")
        q = torch.zeros_like(i)
        self.process(torch.from_numpy(keys).cuda(), i, q)
        self.synchronize()
        return i.cpu().numpy(), q.cpu().numpy()

    def _outputs(self):
        self.synchronize()
        return self._pointers("outputs", 5)

    def flags(self) -> np.ndarray:
        """uint8 [C][blocks] of the last process call"""
        return self._fetch(self._outputs()[0], (self.channels, self._blocks), np.uint8)

    def consumed(self) -> np.ndarray:
        """uint32 [C], characters taken from the queue or discarded by a key closure since reset"""
        return self._fetch(self._outputs()[1], self.channels, np.uint32)

    def echo_total(self) -> np.ndarray:
        """uint32 [C], bytes printed since reset"""
        return self._fetch(self._outputs()[3], self.channels, np.uint32)

    def echo(self) -> list:
        """per channel the last min(echo_total, echo_capacity) bytes printed, oldest first"""
        out = self._outputs()
        ring = self._fetch(out[2], (self.channels, self.echo_capacity), np.uint8)
        total = self._fetch(out[3], self.channels, np.uint32)
        cap = self.echo_capacity
        return [bytes(ring[c, :t]) if t <= cap else bytes(np.roll(ring[c], -(int(t) % cap))) for c, t in enumerate(total)]

    def state(self) -> np.ndarray:
        """uint8 [C], ps.cw_state; in STRAIGHT mode ps.key_timer"""
        return self._fetch(self._outputs()[4], self.channels, np.uint8)

    def peek(self) -> dict:
        """the keyer's words by name (WORDS), uint32 [C] each"""
        self.synchronize()
        p, rows = C.c_void_p(), C.c_int32()
        self._call("peek", C.byref(p), C.byref(rows))
        words = self._fetch(p.value, (rows.value, self.channels), np.uint32)
        return dict(zip(WORDS, words))
