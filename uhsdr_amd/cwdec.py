"""Batched CW decoder back end, Morse to text (uhsdr_cwdec_*, include/uhsdr.h): one decoder per
channel, fed the mark/space byte of every CW block; exact to the firmware's CW_Decode."""
from __future__ import annotations

import numpy as np

from . import _abi
from ._handle import TextDecoder, TextRing

SPIKECANCEL_OFF, SPIKECANCEL_SPIKE, SPIKECANCEL_SHORT = 0, 1, 2


class TextOutputs(TextRing):
    """The decoder's outputs: read() is (text uint8 [C][capacity] ring, total uint32 [C], wpm uint8 [C])."""

    def __init__(self, lib, channels: int, capacity: int, device: bool, text: int, total: int, wpm: int):
        super().__init__(lib, channels, capacity, device, text, total, extra=((wpm, np.uint8),))


class CwDecoder(TextDecoder):
    kind = "cwdec"

    def __init__(self, channels: int, blocksize: int = 88, spikecancel: int = SPIKECANCEL_OFF, text_capacity: int = 64,
                 host: bool = False, stream: int | None = None):
        self.blocksize, self.text_capacity = int(blocksize), int(text_capacity)
        self._create(channels, (self.blocksize, int(spikecancel), self.text_capacity), host, stream)
        self.outputs = TextOutputs(self.lib, self.channels, self.text_capacity, not host, *self._pointers("outputs", 3))

    def process(self, state, blocks: int | None = None) -> None:
        """state: uint8 [C][stride], one byte per CW block, non-zero = mark: a contiguous numpy array
        for a host decoder, a torch cuda tensor for a device one (stream-ordered).  Decodes the first
        `blocks` (default: all) of every row."""
        self._process(state, np.uint8, "state", blocks)


def char_id(code: int) -> int:
    """CwGen_CharacterIdFunc: the character of a two-bits-per-element code (0xfe empty, 0xff unknown)."""
    return int(_abi.load().uhsdr_cwdec_char_id(int(code)))
