"""Host-side mirror of the reference SSB transmit interface for the batched device chain.

    chain = TxChain(config, channels=C, frames=N)   # TxProcessor_Init + TxProcessor_Set
    chain.process(audio_dev, iq_dev, a0_dev)         # N/32 x TX-mode AudioDriver_I2SCallback

``audio`` is [C][N][2] int32 AudioSample_t codec frames, ``iq`` [C][N][2] int32 IqSample_t DAC
frames, ``a0`` optional [C][N] f32 compressed audio (adb.a_buffer[0]).  All arithmetic runs in
libuhsdr_amd.so (uhsdr_tx.hip); torch tensors only provide device memory.
"""
from __future__ import annotations

import ctypes as C

from . import _abi


class TxChain:
    def __init__(self, config: _abi.TxConfig | None = None, channels: int = 1, frames: int = 32,
                 stream: int | None = None, **overrides):
        self.lib = _abi.load()
        self.config = config if config is not None else _abi.default_tx_config(**overrides)
        self.channels, self.frames = int(channels), int(frames)
        h = C.c_void_p()
        _abi.check(self.lib.uhsdr_tx_create(C.byref(self.config), self.channels, self.frames,
                                            C.c_void_p(stream or 0), C.byref(h)), "uhsdr_tx_create")
        self.handle = h
        self.plan = _abi.TxPlan()
        _abi.check(self.lib.uhsdr_tx_get_plan(h, C.byref(self.plan)), "uhsdr_tx_get_plan")

    def reset(self) -> None:
        _abi.check(self.lib.uhsdr_tx_reset(self.handle), "uhsdr_tx_reset")

    def process(self, audio, iq, a0=None) -> None:
        want = (self.channels, self.frames, 2)
        if tuple(audio.shape) != want or tuple(iq.shape) != want:
            raise ValueError(f"audio / iq must be {want}")
        if a0 is not None and tuple(a0.shape) != want[:2]:
            raise ValueError(f"a0 must be {want[:2]}")
        _abi.check(self.lib.uhsdr_tx_process(self.handle, C.c_void_p(audio.data_ptr()), C.c_void_p(iq.data_ptr()),
                                             C.c_void_p(a0.data_ptr() if a0 is not None else 0)), "uhsdr_tx_process")

    def set_pipelined(self, enable: bool) -> None:
        """tx_iq on a side stream, overlapping the next call's tx_voice (uhsdr_tx_set_pipelined);
        call join() before reading iq."""
        _abi.check(self.lib.uhsdr_tx_set_pipelined(self.handle, int(bool(enable))), "uhsdr_tx_set_pipelined")

    @property
    def pipelined(self) -> bool:
        return bool(self.lib.uhsdr_tx_get_pipelined(self.handle))

    def set_precision(self, precision: int) -> None:
        """PRECISION_EXACT (bit-identical, default) or PRECISION_FMA (fused MACs in the Hilbert pair,
        1e-5 normwise on the DAC frames; uhsdr_tx_set_precision)."""
        _abi.check(self.lib.uhsdr_tx_set_precision(self.handle, int(precision)), "uhsdr_tx_set_precision")

    @property
    def precision(self) -> int:
        return self.lib.uhsdr_tx_get_precision(self.handle)

    def join(self) -> None:
        """order the handle's stream after the pipelined mode's side stream (uhsdr_tx_join)"""
        _abi.check(self.lib.uhsdr_tx_join(self.handle), "uhsdr_tx_join")

    def set_tune(self, tune: int) -> None:
        """TUNE for the following calls: TUNE_OFF, TUNE_SINGLE (750 Hz) or TUNE_TWO (750 + 1950 Hz)."""
        _abi.check(self.lib.uhsdr_tx_set_tune(self.handle, int(tune)), "uhsdr_tx_set_tune")

    def set_tone_burst(self, active: bool) -> None:
        """FM tone burst (whistle-up) on / off for the following calls."""
        _abi.check(self.lib.uhsdr_tx_set_tone_burst(self.handle, int(bool(active))), "uhsdr_tx_set_tone_burst")

    # ---- DIGI transmit (dmod_mode DEMOD_DIGI): the modulator inside the chain ----

    def set_rtty_mod(self, enable: bool, shift: int = 1, speed: int = 0, stopbits: int = 1, capacity: int = 128) -> None:
        """the handle's RTTY modulator on / off (uhsdr_tx_set_rtty_mod; arguments as RttyModulator)"""
        _abi.check(self.lib.uhsdr_tx_set_rtty_mod(self.handle, int(bool(enable)), int(shift), int(speed), int(stopbits), int(capacity)),
                   "uhsdr_tx_set_rtty_mod")

    def set_psk_mod(self, enable: bool, speed: int = 0, capacity: int = 128) -> None:
        """the handle's BPSK modulator on / off (uhsdr_tx_set_psk_mod; arguments as PskModulator)"""
        _abi.check(self.lib.uhsdr_tx_set_psk_mod(self.handle, int(bool(enable)), int(speed), int(capacity)), "uhsdr_tx_set_psk_mod")

    def mod_put_text(self, text):
        """text: one bytes object per channel (or one for all); returns the accepted counts int32 [C]"""
        import numpy as np
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
        _abi.check(self.lib.uhsdr_tx_mod_put_text(self.handle, rows.ctypes.data_as(C.c_void_p), length.ctypes.data_as(C.c_void_p),
                                                  stride, accepted.ctypes.data_as(C.c_void_p)), "uhsdr_tx_mod_put_text")
        return accepted

    def mod_start(self) -> None:
        """Rtty_Modulator_StartTX / Psk_Modulator_PrepareTx on every channel"""
        _abi.check(self.lib.uhsdr_tx_mod_start(self.handle), "uhsdr_tx_mod_start")

    def mod_outputs(self):
        """(consumed uint32 [C], txoff_at uint32 [C], state uint8 [C]) as host arrays; the work enqueued must be complete"""
        import numpy as np
        p = [C.c_void_p() for _ in range(3)]
        _abi.check(self.lib.uhsdr_tx_mod_outputs(self.handle, C.byref(p[0]), C.byref(p[1]), C.byref(p[2])), "uhsdr_tx_mod_outputs")
        out = []
        for ptr, dtype in zip(p, (np.uint32, np.uint32, np.uint8)):
            arr = np.empty(self.channels, dtype)
            _abi.check(self.lib.uhsdr_copy_to_host(arr.ctypes.data_as(C.c_void_p), ptr, arr.nbytes), "uhsdr_copy_to_host")
            out.append(arr)
        return tuple(out)

    def process_digi(self, iq, a0=None) -> None:
        """uhsdr_tx_process with a modulator on: no audio input"""
        want = (self.channels, self.frames, 2)
        if tuple(iq.shape) != want or (a0 is not None and tuple(a0.shape) != want[:2]):
            raise ValueError(f"iq must be {want}, a0 {want[:2]}")
        _abi.check(self.lib.uhsdr_tx_process(self.handle, None, C.c_void_p(iq.data_ptr()),
                                             C.c_void_p(a0.data_ptr() if a0 is not None else 0)), "uhsdr_tx_process")

    # ---- CW transmit (dmod_mode DEMOD_CW): the keyer inside the chain ----

    def set_cw_keyer(self, capacity: int = 128, echo_capacity: int = 256) -> None:
        """the handle's CW generator with the config's keyer settings (uhsdr_tx_set_cw_keyer)"""
        _abi.check(self.lib.uhsdr_tx_set_cw_keyer(self.handle, int(capacity), int(echo_capacity)), "uhsdr_tx_set_cw_keyer")
        self._echo_capacity = int(echo_capacity)

    def cw_keys(self, keys) -> None:
        """keys: uint8 cuda tensor [C][frames / 32], read by the following process_cw calls; keep it alive"""
        if keys is not None and (tuple(keys.shape) != (self.channels, self.frames // 32) or keys.element_size() != 1 or not keys.is_contiguous()):
            raise ValueError("keys must be a contiguous uint8 tensor [C][frames / 32]")
        self._keys = keys
        _abi.check(self.lib.uhsdr_tx_cw_keys(self.handle, C.c_void_p(keys.data_ptr() if keys is not None else 0)), "uhsdr_tx_cw_keys")

    def cw_put_text(self, text):
        """text: one bytes object per channel (or one for all); returns the accepted counts int32 [C]"""
        import numpy as np
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
        _abi.check(self.lib.uhsdr_tx_cw_put_text(self.handle, rows.ctypes.data_as(C.c_void_p), length.ctypes.data_as(C.c_void_p),
                                                 stride, accepted.ctypes.data_as(C.c_void_p)), "uhsdr_tx_cw_put_text")
        return accepted

    def cw_set_speed(self, speed: int, weight: int = 100) -> None:
        _abi.check(self.lib.uhsdr_tx_cw_set_speed(self.handle, int(speed), int(weight)), "uhsdr_tx_cw_set_speed")

    def cw_outputs(self):
        """(flags uint8 [C][frames / 32] of the last call, consumed uint32 [C], echo uint8 [C][echo_capacity], echo_total
        uint32 [C], state uint8 [C]) as host arrays; the work enqueued must be complete"""
        import numpy as np
        p = [C.c_void_p() for _ in range(5)]
        _abi.check(self.lib.uhsdr_tx_cw_outputs(self.handle, *(C.byref(x) for x in p)), "uhsdr_tx_cw_outputs")
        shapes = ((self.channels, self.frames // 32), self.channels, (self.channels, self._echo_capacity), self.channels, self.channels)
        out = []
        for ptr, shape, dtype in zip(p, shapes, (np.uint8, np.uint32, np.uint8, np.uint32, np.uint8)):
            arr = np.zeros(shape, dtype)
            if ptr.value:
                _abi.check(self.lib.uhsdr_copy_to_host(arr.ctypes.data_as(C.c_void_p), ptr, arr.nbytes), "uhsdr_copy_to_host")
            out.append(arr)
        return tuple(out)

    def process_cw(self, iq, a0=None) -> None:
        """uhsdr_tx_process on a CW handle: no audio input"""
        self.process_digi(iq, a0)

    def close(self) -> None:
        if self.handle:
            self.lib.uhsdr_tx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
