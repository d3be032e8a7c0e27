"""Batched BPSK decoder, varicode to text (uhsdr_psk_*, include/uhsdr.h): one decoder per channel,
fed 12 ksps audio sample by sample; exact to the firmware's Psk_Demodulator_ProcessSample."""
from __future__ import annotations

import numpy as np

from ._handle import TextDecoder
from .rtty import RttyOutputs

SPEED_31, SPEED_63, SPEED_125 = range(3)


class PskOutputs(RttyOutputs):
    """The decoder's outputs: read() is (text uint8 [C][capacity] ring, total uint32 [C]); the symbol is read apart."""

    def __init__(self, lib, channels: int, capacity: int, device: bool, text: int, total: int, symbol: int):
        super().__init__(lib, channels, capacity, device, text, total)
        self.symbol_ptr = symbol

    def read_symbol(self):
        """symbol float32 [C], rx_last_symbol: the averaged phase at the last bit decision"""
        return self._get(self.symbol_ptr, self.channels, np.float32)


class PskDecoder(TextDecoder):
    kind = "psk"

    def __init__(self, channels: int, speed: int = SPEED_31, capacity: int = 64, host: bool = False, stream: int | None = None):
        self.text_capacity = int(capacity)
        self._create(channels, (int(speed), self.text_capacity), host, stream)
        self.outputs = PskOutputs(self.lib, self.channels, self.text_capacity, not host, *self._pointers("outputs", 3))

    def process(self, samples, n: int | None = None) -> None:
        """samples: float32 [C][stride], 12 ksps audio: a contiguous numpy array for a host decoder, a
        torch cuda tensor for a device one (stream-ordered).  Decodes the first `n` (default: all)
        of every row."""
        self._process(samples, np.float32, "samples", n)

    def symbol(self):
        self.synchronize()
        return self.outputs.read_symbol()
