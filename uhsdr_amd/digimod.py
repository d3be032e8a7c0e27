"""Batched RTTY and BPSK modulators, text to 48 ksps int16 audio (uhsdr_rttymod_*, uhsdr_pskmod_*,
include/uhsdr.h): one modulator and one text queue per channel; exact to the firmware's
Rtty_Modulator_GenSample and Psk_Modulator_GenSample."""
from __future__ import annotations

import numpy as np

from ._handle import TextSender
from .rtty import SHIFT_170, SPEED_45, STOP_1_5
from .psk import SPEED_31

NO_TXOFF = 0xFFFFFFFF
PSK_OFF, PSK_PREAMBLE, PSK_ACTIVE, PSK_POSTAMBLE, PSK_INACTIVE = range(5)
EOT = b"\x04"


class _Modulator(TextSender):
    """What the two have in common."""

    def _create(self, channels: int, args: tuple, capacity: int, host: bool, stream: int | None) -> None:
        self.text_capacity = int(capacity)
        super()._create(channels, (*args, self.text_capacity), host, stream)
        self._out = self._pointers("outputs", 3)

    def process(self, audio, n: int | None = None) -> None:
        """audio: int16 [C][stride]: a contiguous numpy array for a host modulator, a torch cuda tensor
        for a device one (stream-ordered).  Writes the next `n` (default: all) samples of every row."""
        self._process(audio, np.int16, "audio", n)

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

    def _get(self, k: int, dtype):
        self.synchronize()
        return self._fetch(self._out[k], self.channels, dtype)

    def consumed(self) -> np.ndarray:
        """uint32 [C], characters taken from the queue since reset"""
        return self._get(0, np.uint32)

    def txoff_at(self) -> np.ndarray:
        """uint32 [C], the first sample since reset that requested TX-off, NO_TXOFF if none"""
        return self._get(1, np.uint32)

    def state(self) -> np.ndarray:
        """uint8 [C], the BPSK modulator state (PSK_OFF .. PSK_INACTIVE); 0 for RTTY"""
        return self._get(2, np.uint8)


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
