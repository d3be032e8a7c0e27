"""Batched RTTY decoder, Baudot to text (uhsdr_rtty_*, include/uhsdr.h): one decoder per channel,
fed 12 ksps audio sample by sample; exact to the firmware's Rtty_Demodulator_ProcessSample."""
from __future__ import annotations

import numpy as np

from ._handle import TextDecoder, TextRing

SHIFT_85, SHIFT_170, SHIFT_200, SHIFT_425, SHIFT_450, SHIFT_850 = range(6)
SPEED_45, SPEED_50 = range(2)
STOP_1, STOP_1_5, STOP_2 = range(3)


class RttyOutputs(TextRing):
    """The decoder's outputs: read() is (text uint8 [C][capacity] ring, total uint32 [C])."""


class RttyDecoder(TextDecoder):
    kind = "rtty"

    def __init__(self, channels: int, shift: int = SHIFT_170, speed: int = SPEED_45, stopbits: int = STOP_1_5,
                 atc_disable: bool = False, capacity: int = 64, host: bool = False, stream: int | None = None):
        self.text_capacity = int(capacity)
        self._create(channels, (int(shift), int(speed), int(stopbits), int(bool(atc_disable)), self.text_capacity), host, stream)
        self.outputs = RttyOutputs(self.lib, self.channels, self.text_capacity, not host, *self._pointers("outputs", 2))

    def process(self, samples, n: int | None = None) -> None:
        """samples: float32 [C][stride], 12 ksps audio: a contiguous numpy array for a host decoder, a
        torch cuda tensor for a device one (stream-ordered).  Decodes the first `n` (default: all)
        of every row."""
        self._process(samples, np.float32, "samples", n)
