"""Host-side mirror of the reference spectrum display path for the batched device kernel.

    spec = Spectrum(config, channels=C, frames=N)   # UiSpectrum_InitSpectrumDisplayData
    nf = spec.process(iq_dev, mag_dev, avg_dev)     # N input frames: producer ring + states 0-3

``iq`` is the RX input, [C][N][2] int32 IqSample_t; ``mag`` / ``avg`` are optional [C][F][L] f32
(F = max(1, N/L)): sd.FFT_MagData and sd.FFT_AVGData after each display frame completed by the
call; ``nf`` is how many were completed.  ``spec.set_meter(meter, dbm=..., s_count=...)`` adds the
signal meter's outputs per completed frame, ``spec.set_display(display, scope=..., wfall=...)`` the
display stage's scope trace and waterfall line.  All arithmetic runs in libuhsdr_amd.so
(uhsdr_spectrum.hip); torch tensors only provide device memory.
"""
from __future__ import annotations

import ctypes as C

from . import _abi


class Spectrum:
    def __init__(self, config: _abi.SpectrumConfig | None = None, channels: int = 1, frames: int = 1024,
                 stream: int | None = None, **overrides):
        self.lib = _abi.load()
        self.config = config if config is not None else _abi.default_spectrum_config(**overrides)
        self.channels, self.frames = int(channels), int(frames)
        h = C.c_void_p()
        _abi.check(self.lib.uhsdr_spectrum_create(C.byref(self.config), self.channels, self.frames,
                                                  C.c_void_p(stream or 0), C.byref(h)), "uhsdr_spectrum_create")
        self.handle = h
        self.plan = _abi.SpectrumPlan()
        _abi.check(self.lib.uhsdr_spectrum_get_plan(h, C.byref(self.plan)), "uhsdr_spectrum_get_plan")
        self.fft_len = self.plan.fft_len
        self.decimation = 1 << int(self.config.magnify)          # zoom: ring samples per frame
        self.frames_out = max(1, self.frames // self.decimation // self.fft_len)

    @property
    def out_shape(self):
        return (self.channels, self.frames_out, self.fft_len)

    def reset(self) -> None:
        _abi.check(self.lib.uhsdr_spectrum_reset(self.handle), "uhsdr_spectrum_reset")

    def process(self, iq, mag=None, avg=None) -> int:
        if tuple(iq.shape) != (self.channels, self.frames, 2):
            raise ValueError(f"iq must be {(self.channels, self.frames, 2)}")
        for t in (mag, avg):
            if t is not None and tuple(t.shape) != self.out_shape:
                raise ValueError(f"mag / avg must be {self.out_shape}")
        nf = C.c_int32(0)
        _abi.check(self.lib.uhsdr_spectrum_process(
            self.handle, C.c_void_p(iq.data_ptr()), C.c_void_p(mag.data_ptr() if mag is not None else 0),
            C.c_void_p(avg.data_ptr() if avg is not None else 0), C.byref(nf)), "uhsdr_spectrum_process")
        return nf.value

    def set_meter(self, meter, cw_signal=None, **rows) -> None:
        """Attach a device Meter (uhsdr_amd.meter): every process() then runs the meter's frame on each
        display frame it completes and writes `rows`, cuda tensors [C][frames_out] named as
        meter.OUTPUTS; mag and avg may then both be None.  None detaches.  The spectrum keeps a
        reference to the meter and the rows while attached."""
        if meter is None:
            _abi.check(self.lib.uhsdr_spectrum_set_meter(self.handle, None, None), "uhsdr_spectrum_set_meter")
            self._meter = None
            return
        io = meter.io(self.frames_out, cw_signal, **rows)
        _abi.check(self.lib.uhsdr_spectrum_set_meter(self.handle, meter.handle, C.byref(io)), "uhsdr_spectrum_set_meter")
        self._meter = (meter, cw_signal, rows)

    def set_display(self, display, **rows) -> None:
        """Attach a device Display (uhsdr_amd.display): every process() then runs the display stage's
        frame on each display frame it completes, after the meter's, and writes `rows`, cuda tensors
        named as display.OUTPUTS ([C][frames_out][width] and [C][frames_out]); mag and avg may then
        both be None.  None detaches.  The spectrum keeps a reference to the display and the rows
        while attached."""
        if display is None:
            _abi.check(self.lib.uhsdr_spectrum_set_display(self.handle, None, None), "uhsdr_spectrum_set_display")
            self._display = None
            return
        io = display.io(self.frames_out, **rows)
        _abi.check(self.lib.uhsdr_spectrum_set_display(self.handle, display.handle, C.byref(io)), "uhsdr_spectrum_set_display")
        self._display = (display, rows)

    def close(self) -> None:
        if self.handle:
            self._meter = None
            self._display = None
            self.lib.uhsdr_spectrum_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
