"""Batched noise blanker (uhsdr_nb_*, include/uhsdr.h): one instance per channel, fed the 128-sample
frames of the noise reduction; exact to the firmware's alt_noise_blanking.  The blanker inside the
12 ksps stream is NrProcessor with nb_setting (and nr_bypass for the blanker alone)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._handle import Handle

FRAME = 128          # samples per frame
DELAY = 13           # a frame's output lags its input by this many samples
MAX_HITS = 5         # places repaired per frame at most
REPAIR = 7           # samples per repaired place


def nb_config(**overrides) -> _abi.NbConfig:
    """uhsdr_nb_config_default with fields replaced"""
    cfg = _abi.NbConfig()
    _abi.load().uhsdr_nb_config_default(C.byref(cfg))
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


class NbProcessor(Handle):
    kind = "nb"

    def __init__(self, channels: int, cfg: _abi.NbConfig | None = None, host: bool = False, stream: int | None = None):
        self.cfg = cfg if cfg is not None else nb_config()
        self._create(channels, (C.byref(self.cfg),), host, stream)

    def process_frames(self, x, out=None, frames: int | None = None) -> None:
        """x, out: float32 [C][stride], numpy arrays for a host processor, torch cuda tensors for a
        device one (stream-ordered); runs the first `frames` (default: all whole) frames of every
        row.  out None or x itself: in place."""
        pi, stride = self.rows(x, np.float32, "x")
        po = pi
        if out is not None and out is not x:
            po, so = self.rows(out, np.float32, "out")
            if so != stride:
                raise ValueError("in and out must have one stride")
        self._call("process_frames_host" if self.host else "process_frames", pi, po, stride // FRAME if frames is None else int(frames), stride)

    def state(self):
        """(places repaired in the last frame int32 [C], since the reset uint32 [C]) after everything enqueued"""
        last, total = np.empty(self.channels, np.int32), np.empty(self.channels, np.uint32)
        self._call("state", last.ctypes.data_as(C.c_void_p), total.ctypes.data_as(C.c_void_p))
        return last, total
