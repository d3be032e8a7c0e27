"""Synthetic 48 kHz I/Q workloads.

Every channel is an independent radio receiving a two-tone SSB signal that sits at
+12 kHz in the I/Q spectrum (so the default ``iq_freq_mode`` = -12 kHz conversion,
audio_driver.h:526 / freq_shift.c:219-262, brings it to baseband) plus white noise.
Samples are delivered exactly as the codec DMA delivers them to
``AudioDriver_RxProcessor`` (audio_driver.c:2660-2685): interleaved ``IqSample_t``
``{int32 l, int32 r}`` frames holding ``(int16) value << 16``.

All randomness is counter-based (splitmix64 of (channel seed, sample index)), so the
samples of channel ``c`` do not depend on how many channels are generated or in which
chunks — a 4-channel fixture and a 4096-channel bench batch agree on channel 0..3.
"""
from __future__ import annotations

import numpy as np

FS = 48000.0
SEED_BASE = 0x5EED0000
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x: np.ndarray) -> np.ndarray:
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
    z = x
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
    return z ^ (z >> np.uint64(31))


def _uniform(key: np.ndarray) -> np.ndarray:
    """(0, 1) doubles from 64-bit keys."""
    return ((_splitmix64(key) >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def channel_params(channels: np.ndarray, kind: str = "ssb2tone"):
    """Per-channel tone parameters (frequencies in Hz relative to the +12 kHz carrier)."""
    ch = channels.astype(np.uint64)
    base = (np.uint64(SEED_BASE) + ch) << np.uint64(20)
    u = [_uniform(base + np.uint64(k)) for k in range(6)]
    if kind == "c1":   # C1: fixed 700 + 1900 Hz, peak 3000 LSB16 (1500 each)
        f1 = np.full(ch.shape, 700.0)
        f2 = np.full(ch.shape, 1900.0)
        a1 = np.full(ch.shape, 1500.0)
        a2 = np.full(ch.shape, 1500.0)
    else:              # C2: audio tones in [300, 2500] Hz, summed peak in [300, 3000] LSB16
        f1 = 300.0 + 2200.0 * u[0]
        f2 = 300.0 + 2200.0 * u[1]
        a1 = 150.0 + 1350.0 * u[2]
        a2 = 150.0 + 1350.0 * u[3]
    p1 = 2.0 * np.pi * u[4]
    p2 = 2.0 * np.pi * u[5]
    return f1, f2, a1, a2, p1, p2


def ssb_iq(channels, start: int, nframes: int, kind: str = "ssb2tone",
           noise_sigma: float = 30.0, lsb: bool = False, carrier: float = 12000.0) -> np.ndarray:
    """int32 frames, shape [len(channels), nframes, 2] = {l (I), r (Q)} per IqSample_t.

    Sample index ``start + i`` is absolute, so consecutive calls continue the stream.
    ``carrier`` is where the suppressed carrier sits in the I/Q spectrum: +12 kHz for the
    default -12 kHz conversion, -12/+-6/0 kHz for the other FREQ_IQ_CONV modes.
    """
    channels = np.asarray(channels, dtype=np.int64)
    f1, f2, a1, a2, p1, p2 = channel_params(channels, kind)
    sgn = -1.0 if lsb else 1.0
    n = np.arange(start, start + nframes, dtype=np.float64)[None, :]
    w1 = 2.0 * np.pi * (carrier + sgn * f1[:, None]) / FS
    w2 = 2.0 * np.pi * (carrier + sgn * f2[:, None]) / FS
    ph1 = w1 * n + p1[:, None]
    ph2 = w2 * n + p2[:, None]
    i_sig = a1[:, None] * np.cos(ph1) + a2[:, None] * np.cos(ph2)
    q_sig = a1[:, None] * np.sin(ph1) + a2[:, None] * np.sin(ph2)
    if noise_sigma > 0:
        ch = channels.astype(np.uint64)[:, None]
        idx = np.arange(start, start + nframes, dtype=np.uint64)[None, :]
        key = ((np.uint64(SEED_BASE) + ch) << np.uint64(40)) ^ (idx << np.uint64(1))
        u1 = _uniform(key)
        u2 = _uniform(key ^ np.uint64(1))
        r = np.sqrt(-2.0 * np.log(u1)) * noise_sigma
        i_sig = i_sig + r * np.cos(2.0 * np.pi * u2)
        q_sig = q_sig + r * np.sin(2.0 * np.pi * u2)
    out = np.empty((len(channels), nframes, 2), dtype=np.int32)
    out[:, :, 0] = np.clip(np.rint(i_sig), -32768, 32767).astype(np.int32) << 16
    out[:, :, 1] = np.clip(np.rint(q_sig), -32768, 32767).astype(np.int32) << 16
    return out


def _noise(channels, start, nframes, noise_sigma):
    ch = channels.astype(np.uint64)[:, None]
    idx = np.arange(start, start + nframes, dtype=np.uint64)[None, :]
    key = ((np.uint64(SEED_BASE) + ch) << np.uint64(40)) ^ (idx << np.uint64(1))
    u1 = _uniform(key)
    u2 = _uniform(key ^ np.uint64(1))
    r = np.sqrt(-2.0 * np.log(u1)) * noise_sigma
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def _frames(i_sig, q_sig):
    out = np.empty(i_sig.shape + (2,), dtype=np.int32)
    out[..., 0] = np.clip(np.rint(i_sig), -32768, 32767).astype(np.int32) << 16
    out[..., 1] = np.clip(np.rint(q_sig), -32768, 32767).astype(np.int32) << 16
    return out


def am_iq(channels, start: int, nframes: int, noise_sigma: float = 30.0, carrier: float = 12000.0,
          depth: float = 0.5, tone: float = 1000.0, amplitude: float = 2000.0, offset_hz: float = 200.0):
    """C3: AM, carrier at `carrier` + U(-offset_hz, offset_hz) Hz per channel,
    `depth` modulation with a `tone` Hz audio tone, peak carrier `amplitude` LSB16, plus noise.
    The SAM PLL has to acquire and track each channel's carrier offset."""
    channels = np.asarray(channels, dtype=np.int64)
    ch = channels.astype(np.uint64)
    base = (np.uint64(SEED_BASE) + ch) << np.uint64(20)
    off = offset_hz * (2.0 * _uniform(base + np.uint64(7)) - 1.0)
    ph_c = 2.0 * np.pi * _uniform(base + np.uint64(8))
    ph_m = 2.0 * np.pi * _uniform(base + np.uint64(9))
    n = np.arange(start, start + nframes, dtype=np.float64)[None, :]
    env = amplitude * (1.0 + depth * np.cos(2.0 * np.pi * tone / FS * n + ph_m[:, None]))
    ph = 2.0 * np.pi * (carrier + off[:, None]) / FS * n + ph_c[:, None]
    i_sig, q_sig = env * np.cos(ph), env * np.sin(ph)
    if noise_sigma > 0:
        ni, nq = _noise(channels, start, nframes, noise_sigma)
        i_sig, q_sig = i_sig + ni, q_sig + nq
    return _frames(i_sig, q_sig)


def cw_iq(channels, start: int, nframes: int, noise_sigma: float = 30.0, carrier: float = 12000.0,
          tone: float = 750.0, amplitude: float = 1500.0, element: int = 2400):
    """C5 CW: an on/off keyed carrier at `carrier` + `tone` +- 40 Hz per
    channel (the receiver's sidetone pitch), keyed in elements of `element` frames (50 ms =
    24 wpm at 48 ksps) with a per-channel pseudo-random pattern, plus noise."""
    channels = np.asarray(channels, dtype=np.int64)
    ch = channels.astype(np.uint64)
    base = (np.uint64(SEED_BASE) + ch) << np.uint64(20)
    off = 40.0 * (2.0 * _uniform(base + np.uint64(11)) - 1.0)
    ph_c = 2.0 * np.pi * _uniform(base + np.uint64(12))
    n = np.arange(start, start + nframes, dtype=np.float64)[None, :]
    el = (np.arange(start, start + nframes) // element).astype(np.uint64)[None, :]
    key = _uniform((base[:, None] + np.uint64(1 << 19)) + el) < 0.55
    ph = 2.0 * np.pi * (carrier + tone + off[:, None]) / FS * n + ph_c[:, None]
    i_sig, q_sig = amplitude * key * np.cos(ph), amplitude * key * np.sin(ph)
    if noise_sigma > 0:
        ni, nq = _noise(channels, start, nframes, noise_sigma)
        i_sig, q_sig = i_sig + ni, q_sig + nq
    return _frames(i_sig, q_sig)


def fm_iq(channels, start: int, nframes: int, noise_sigma: float = 30.0, carrier: float = 12000.0,
          deviation: float = 2500.0, tone: float = 1000.0, amplitude: float = 3000.0,
          subtone: float = 0.0, subtone_dev: float = 300.0):
    """C4 FM-RX: carrier at `carrier` Hz, a `tone` Hz audio tone at
    `deviation` Hz peak deviation, `amplitude` LSB16, plus noise; optionally a CTCSS
    subaudible tone of `subtone` Hz at `subtone_dev` Hz deviation (the FM tone detector's
    input, audio_driver.c:1665-1734)."""
    channels = np.asarray(channels, dtype=np.int64)
    ch = channels.astype(np.uint64)
    base = (np.uint64(SEED_BASE) + ch) << np.uint64(20)
    ph_c = 2.0 * np.pi * _uniform(base + np.uint64(10))
    ph_m = 2.0 * np.pi * _uniform(base + np.uint64(11))
    n = np.arange(start, start + nframes, dtype=np.float64)[None, :]
    ph = (2.0 * np.pi * carrier / FS * n + ph_c[:, None]
          + (deviation / tone) * np.sin(2.0 * np.pi * tone / FS * n + ph_m[:, None]))
    if subtone > 0:
        ph = ph + (subtone_dev / subtone) * np.sin(2.0 * np.pi * subtone / FS * n)
    i_sig, q_sig = amplitude * np.cos(ph), amplitude * np.sin(ph)
    if noise_sigma > 0:
        ni, nq = _noise(channels, start, nframes, noise_sigma)
        i_sig, q_sig = i_sig + ni, q_sig + nq
    return _frames(i_sig, q_sig)


STATUS_PHASE_DEG = (0.0, 12.0, 30.0, 60.0, 89.0)


def status_iq(channels, start: int, nframes: int, noise_sigma: float = 30.0, burst_every: int = 3000,
              burst_len: int = 256):
    """Status side outputs (ADC clip flags, twin-peaks detector; audio_driver.c:2660-2676,
    2173-2248): the two-tone SSB signal of ``ssb_iq`` with an I/Q phase error of
    STATUS_PHASE_DEG[channel % 5] degrees on Q (Q = A sin(theta + phi); the Moseley & Slump
    estimate asin(teta1 / teta3) sees -phi), and every `burst_every` frames a `burst_len`-frame
    burst at 1.5 + (channel*7 + k) % 6 times the level, so |I| crosses the quarter / half / full
    ADC clip thresholds (1024 / 2048 / 4096 LSB16) on different calls per channel.  Peak stays
    below 32767 (no full-scale samples)."""
    channels = np.asarray(channels, dtype=np.int64)
    f1, f2, a1, a2, p1, p2 = channel_params(channels, "ssb2tone")
    phi = np.deg2rad(np.array(STATUS_PHASE_DEG)[channels % len(STATUS_PHASE_DEG)])[:, None]
    n = np.arange(start, start + nframes, dtype=np.float64)[None, :]
    k = (np.arange(start, start + nframes) // burst_every)[None, :]
    inb = (np.arange(start, start + nframes) % burst_every) < burst_len
    gain = np.where(inb[None, :], 1.5 + ((channels[:, None] * 7 + k) % 6), 1.0)
    ph1 = 2.0 * np.pi * (12000.0 + f1[:, None]) / FS * n + p1[:, None]
    ph2 = 2.0 * np.pi * (12000.0 + f2[:, None]) / FS * n + p2[:, None]
    i_sig = gain * (a1[:, None] * np.cos(ph1) + a2[:, None] * np.cos(ph2))
    q_sig = gain * (a1[:, None] * np.sin(ph1 + phi) + a2[:, None] * np.sin(ph2 + phi))
    if noise_sigma > 0:
        ni, nq = _noise(channels, start, nframes, noise_sigma)
        i_sig, q_sig = i_sig + ni, q_sig + nq
    return _frames(i_sig, q_sig)


def tx_audio(channels, start: int, nframes: int, kind: str = "ssb2tone", noise_sigma: float = 10.0):
    """C4 SSB-TX input: the codec's microphone frames (AudioSample_t {int32 l, r}, the sample in
    both channels as (int16) value << 16) carrying a per-channel two-tone audio signal."""
    channels = np.asarray(channels, dtype=np.int64)
    f1, f2, a1, a2, p1, p2 = channel_params(channels, kind)
    n = np.arange(start, start + nframes, dtype=np.float64)[None, :]
    s = (a1[:, None] * np.cos(2.0 * np.pi * f1[:, None] / FS * n + p1[:, None])
         + a2[:, None] * np.cos(2.0 * np.pi * f2[:, None] / FS * n + p2[:, None]))
    if noise_sigma > 0:
        s = s + _noise(channels, start, nframes, noise_sigma)[0]
    return _frames(s, s)


# Edge inputs: silence, signal / silence / signal (the recursive stages decay through the
# denormals and sit there until the signal returns), full-scale samples, all 32 bits in use
EDGE_KINDS = ("zeros", "burst", "impulse", "rails", "lsb", "lowbits")
EDGE_LEAD, EDGE_GAP = 8192, 196608
EDGE_FRAMES = EDGE_LEAD + EDGE_GAP + 4096            # 208896 = 102 x 2048
EDGE_IMPULSE_EVERY = 4099
EDGE_AUDIO_KINDS = ("zeros", "burst", "rails")
EDGE_AUDIO_LEAD, EDGE_AUDIO_GAP = 2048, 131072
EDGE_AUDIO_FRAMES = EDGE_AUDIO_LEAD + EDGE_AUDIO_GAP + 2048   # 135168 = 528 x 256
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def _uniform_int(channels, start, nframes, lo, hi, salt):
    """integers in [lo, hi] per (channel, sample index, I / Q), counter-based; [C, n, 2] int64"""
    ch = np.asarray(channels).astype(np.uint64)[:, None, None]
    idx = np.arange(start, start + nframes, dtype=np.uint64)[None, :, None]
    iq = np.arange(2, dtype=np.uint64)[None, None, :]
    key = ((np.uint64(SEED_BASE) + ch) << np.uint64(40)) ^ (np.uint64(salt) << np.uint64(36)) ^ (idx << np.uint64(1)) ^ iq
    return lo + np.floor(_uniform(key) * (hi - lo + 1)).astype(np.int64)


def _rails(n):
    return np.where((n // 5) % 2 == 0, INT32_MAX, INT32_MIN)


def edge_iq(kind: str, channels, start: int, nframes: int, base=None, shift=0, lead: int = EDGE_LEAD,
            gap: int = EDGE_GAP, **base_kw) -> np.ndarray:
    """int32 I/Q frames [len(channels), nframes, 2] at the edges of the input range, absolute in
    `start` like the others.  `base` (ssb_iq by default, am_iq, fm_iq; `base_kw` goes to it) is
    the signal of the kinds that carry one:

      zeros    silence from the first sample
      burst    `base` for `lead` frames, zeros for `gap` frames, `base` again; the sample index
               runs on across the gap.  `shift` (a number, or one per channel) starts the
               silence that many frames later; it ends at lead + gap all the same
      impulse  I = INT32_MIN at every 4099th frame, Q = INT32_MAX 2048 frames after each of
               those; all zero after frame lead + 2 * 4099
      rails    I alternates between INT32_MAX and INT32_MIN every 5 frames, Q the same 2 frames later
      lsb      uniform integers in [-3, 3], not shifted up: |x| <= 4.6e-5 after the 2^-16 scaling
      lowbits  9 x `base` plus uniform integers in [-32768, 32767], clipped to int32: every one
               of the 32 bits in use, loud enough to wrap the codec frames with the AGC off
    """
    channels = np.asarray(channels, dtype=np.int64)
    base = ssb_iq if base is None else base
    n = np.arange(start, start + nframes, dtype=np.int64)
    out = np.zeros((len(channels), nframes, 2), dtype=np.int32)
    if kind == "zeros":
        pass
    elif kind == "burst":
        sh = np.broadcast_to(np.asarray(shift, dtype=np.int64), channels.shape)
        quiet = (n[None, :] >= lead + sh[:, None]) & (n[None, :] < lead + gap)
        out = np.where(quiet[:, :, None], 0, base(channels, start, nframes, **base_kw)).astype(np.int32)
    elif kind == "impulse":
        on = n <= lead + 2 * EDGE_IMPULSE_EVERY
        out[:, on & (n % EDGE_IMPULSE_EVERY == 0), 0] = INT32_MIN
        out[:, on & (n >= 2048) & ((n - 2048) % EDGE_IMPULSE_EVERY == 0), 1] = INT32_MAX
    elif kind == "rails":
        out[:, :, 0] = _rails(n)[None, :]
        out[:, :, 1] = _rails(n - 2)[None, :]
    elif kind == "lsb":
        out = _uniform_int(channels, start, nframes, -3, 3, 1).astype(np.int32)
    elif kind == "lowbits":
        loud = base(channels, start, nframes, **base_kw).astype(np.int64) * 9
        out = np.clip(loud + _uniform_int(channels, start, nframes, -32768, 32767, 2), INT32_MIN, INT32_MAX).astype(np.int32)
    else:
        raise ValueError(f"edge_iq: unknown kind {kind!r}")
    return out


def edge_audio(kind: str, channels, start: int, nframes: int, lead: int = EDGE_AUDIO_LEAD,
               gap: int = EDGE_AUDIO_GAP) -> np.ndarray:
    """Edge inputs of the transmit chain, codec frames [len(channels), nframes, 2] with the sample
    in both channels: `zeros`; `burst`, tx_audio for `lead` frames, `gap` frames of silence,
    tx_audio again; `rails`, INT32_MAX / INT32_MIN alternating every 5 frames."""
    channels = np.asarray(channels, dtype=np.int64)
    n = np.arange(start, start + nframes, dtype=np.int64)
    out = np.zeros((len(channels), nframes, 2), dtype=np.int32)
    if kind == "zeros":
        pass
    elif kind == "burst":
        quiet = (n >= lead) & (n < lead + gap)
        out = np.where(quiet[None, :, None], 0, tx_audio(channels, start, nframes)).astype(np.int32)
    elif kind == "rails":
        out[:, :, :] = _rails(n)[None, :, None]
    else:
        raise ValueError(f"edge_audio: unknown kind {kind!r}")
    return out


CLIP_RAIL_FRAMES = 2048
# (first frame, I value) of the 256-frame (8-call) stretches of clip_rail_iq
CLIP_RAIL_STRETCHES = ((256, INT32_MIN), (768, -INT32_MAX), (1280, INT32_MAX))


def clip_rail_iq(channels, start: int, nframes: int) -> np.ndarray:
    """The clip flags at the rails: ssb_iq with I held at INT32_MIN for frames [256, 512), at
    -(2^31-1) for [768, 1024) and at INT32_MAX for [1280, 1536).  The reference takes abs() of a
    signed int32, so the first stretch alone raises no flag (audio_driver.c:2662)."""
    out = ssb_iq(channels, start, nframes)
    n = np.arange(start, start + nframes)
    for first, value in CLIP_RAIL_STRETCHES:
        out[:, (n >= first) & (n < first + 256), 0] = value
    return out


def ssb_iq_torch(c0: int, nch: int, start: int, nframes: int, device, noise_sigma: float = 30.0):
    """Same signal model as ``ssb_iq`` (kind "ssb2tone"), generated on the GPU for large
    benchmark batches: channels c0 .. c0+nch-1.  Tone parameters and noise come from the
    same splitmix64 counters; the float64 transcendentals are the device's, so a sample may
    differ from the numpy version by one LSB16 of rounding -- benchmark input only, parity
    tests use ``ssb_iq``."""
    import torch
    f1, f2, a1, a2, p1, p2 = (torch.from_numpy(x).to(device) for x in channel_params(np.arange(c0, c0 + nch)))
    n = torch.arange(start, start + nframes, dtype=torch.float64, device=device)[None, :]
    ph1 = (2.0 * np.pi * (12000.0 + f1[:, None]) / FS) * n + p1[:, None]
    ph2 = (2.0 * np.pi * (12000.0 + f2[:, None]) / FS) * n + p2[:, None]
    i_sig = a1[:, None] * torch.cos(ph1) + a2[:, None] * torch.cos(ph2)
    q_sig = a1[:, None] * torch.sin(ph1) + a2[:, None] * torch.sin(ph2)
    del ph1, ph2
    if noise_sigma > 0:
        g = torch.Generator(device=device)
        g.manual_seed(SEED_BASE + c0 * 7919 + start)
        i_sig += noise_sigma * torch.randn(i_sig.shape, dtype=torch.float64, device=device, generator=g)
        q_sig += noise_sigma * torch.randn(q_sig.shape, dtype=torch.float64, device=device, generator=g)
    out = torch.empty((nch, nframes, 2), dtype=torch.int32, device=device)
    out[:, :, 0] = torch.clamp(torch.round(i_sig), -32768, 32767).to(torch.int32) * 65536
    out[:, :, 1] = torch.clamp(torch.round(q_sig), -32768, 32767).to(torch.int32) * 65536
    return out


# International Morse code (ITU-R M.1677-1): letters, figures, punctuation
MORSE = {
    "A": ".-", "B": "-...", "C": "-.-.", "D": "-..", "E": ".", "F": "..-.", "G": "--.", "H": "....",
    "I": "..", "J": ".---", "K": "-.-", "L": ".-..", "M": "--", "N": "-.", "O": "---", "P": ".--.",
    "Q": "--.-", "R": ".-.", "S": "...", "T": "-", "U": "..-", "V": "...-", "W": ".--", "X": "-..-",
    "Y": "-.--", "Z": "--..",
    "1": ".----", "2": "..---", "3": "...--", "4": "....-", "5": ".....", "6": "-....", "7": "--...",
    "8": "---..", "9": "----.", "0": "-----",
    "=": "-...-", "/": "-..-.", "?": "..--..", '"': ".-..-.", ".": ".-.-.-", "@": ".--.-.", "'": ".----.",
    "-": "-....-", ",": "--..--", ":": "---...",
}


def morse_keying(text: str):
    """The message as (key down?, dot units) runs with PARIS timing: dot 1, dash 3, 1 between the
    elements of a character, 3 between characters, 7 between words; ends with a word space.
    ``<AR>`` sends the letters between the brackets run together (a prosign), ``<HH>`` the
    eight-dot error sign."""
    runs = []
    i = 0
    text = text.upper()
    while i < len(text):
        ch = text[i]
        if ch == " ":
            if runs:
                runs[-1] = (False, 7)
            i += 1
            continue
        if ch == "<":
            j = text.index(">", i)
            pattern = "".join(MORSE[c] for c in text[i + 1:j])
            i = j + 1
        else:
            pattern = MORSE[ch]
            i += 1
        for el in pattern:
            runs.append((True, 3 if el == "-" else 1))
            runs.append((False, 1))
        runs[-1] = (False, 3)
    if runs:
        runs[-1] = (False, 7)
    return runs


def morse_envelope(text: str, wpm: float, rate: float) -> np.ndarray:
    """0/1 key state per sample at `rate` samples per second; a dot lasts 1.2 / wpm seconds."""
    unit = 1.2 / wpm * rate
    edges = np.rint(np.cumsum([0.0] + [u * unit for _, u in morse_keying(text)])).astype(np.int64)
    env = np.zeros(int(edges[-1]), dtype=np.uint8)
    for (down, _), a, b in zip(morse_keying(text), edges[:-1], edges[1:]):
        if down:
            env[a:b] = 1
    return env


def cw_text_iq(channels, start: int, nframes: int, text: str, wpm: float = 20.0, noise_sigma: float = 30.0,
               carrier: float = 12000.0, tone: float = 750.0, amplitude: float = 1500.0, lead: int = 24000):
    """A carrier at `carrier` + `tone` Hz (the receiver's sidetone pitch) keyed with `text` in
    Morse code at `wpm` words per minute, repeated for ever, after `lead` frames of silence plus
    a per-channel delay of up to one second; plus noise.  The CW text decoder's input."""
    channels = np.asarray(channels, dtype=np.int64)
    ch = channels.astype(np.uint64)
    base = (np.uint64(SEED_BASE) + ch) << np.uint64(20)
    delay = lead + np.floor(FS * _uniform(base + np.uint64(13))).astype(np.int64)
    ph_c = 2.0 * np.pi * _uniform(base + np.uint64(12))
    env = morse_envelope(text, wpm, FS)
    reps = nframes // len(env) + 2
    # cos / sin of the common phase once, turned by each channel's start phase
    ph = 2.0 * np.pi * (carrier + tone) / FS * np.arange(start, start + nframes, dtype=np.float64)
    c0, s0 = amplitude * np.cos(ph), amplitude * np.sin(ph)
    i_sig = np.zeros((len(channels), nframes))
    q_sig = np.zeros((len(channels), nframes))
    for k in range(len(channels)):
        first = max(int(delay[k]) - start, 0)          # frames of this call before the channel's keying starts
        if first >= nframes:
            continue
        key = np.tile(env, reps)[(start + first - int(delay[k])) % len(env):][:nframes - first] != 0
        cc, sc = np.cos(ph_c[k]), np.sin(ph_c[k])
        i_sig[k, first:] = np.where(key, c0[first:] * cc - s0[first:] * sc, 0.0)
        q_sig[k, first:] = np.where(key, s0[first:] * cc + c0[first:] * sc, 0.0)
    if noise_sigma > 0:
        ni, nq = _noise(channels, start, nframes, noise_sigma)
        i_sig, q_sig = i_sig + ni, q_sig + nq
    return _frames(i_sig, q_sig)


# ITA2 (Baudot-Murray) as the RTTY decoder prints it: code -> character in the letters and the
# figures case; 27 selects figures, 31 letters, and 0, 2, 4 and 8 read the same in both
BAUDOT_LETTERS = "\0E\nA SIU\rDRJNFCKTZLWHYPQOBG\x0eMXV\x0f"
BAUDOT_FIGURES = "\0" "3\n- \a87\r$4',!:(5\")2#6019?&\x0e./;\x0f"
BAUDOT_FIGS, BAUDOT_LTRS = 27, 31
RTTY_SHIFTS = (85.0, 170.0, 200.0, 425.0, 450.0, 850.0)      # shift_idx 0 .. 5
RTTY_SPEEDS = (45.45, 50.0)                                  # speed_idx 0 .. 1
RTTY_STOPBITS = (1.0, 1.5, 2.0)                              # stopbits_idx 0 .. 2
RTTY_MARK = 915.0


def baudot_codes(text: str, close: bool = False):
    """The 5-bit codes that send `text` (upper-cased), starting in the letters case, with a FIGS
    or LTRS code wherever the case changes; `close` ends in the letters case, so the message can
    be repeated."""
    codes, figs = [], False
    for ch in text.upper():
        in_l, in_f = BAUDOT_LETTERS.find(ch), BAUDOT_FIGURES.find(ch)
        if ch in "\x0e\x0f" or (in_l < 0 and in_f < 0):
            raise ValueError(f"{ch!r} has no Baudot code")
        if (in_f if figs else in_l) < 0:
            figs = not figs
            codes.append(BAUDOT_FIGS if figs else BAUDOT_LTRS)
        codes.append(in_f if figs else in_l)
    if close and figs:
        codes.append(BAUDOT_LTRS)
    return codes


def baudot_bits(text: str, stopbits: float = 1.5, close: bool = False):
    """(level uint8 [k], length float [k]): the line as runs of mark (1) and space (0), lengths in
    bit times: per code a start bit (space), five data bits, lowest first, and `stopbits` of mark."""
    level, length = [], []
    for code in baudot_codes(text, close):
        level += [0] + [(code >> b) & 1 for b in range(5)] + [1]
        length += [1.0] * 6 + [float(stopbits)]
    return np.array(level, np.uint8), np.array(length, np.float64)


def _rtty_line(bits, baud: float, rate: float):
    """mark / space per sample of one pass of the message at `rate` samples per second"""
    level, length = bits
    edges = np.rint(np.cumsum(np.concatenate([[0.0], length * (rate / baud)]))).astype(np.int64)
    return np.repeat(level, np.diff(edges)).astype(np.uint8)


def rtty_audio(text, shift: float = 170.0, baud: float = 45.45, stopbits: float = 1.5, amplitude: float = 1000.0,
               noise_sigma: float = 0.0, fade: str | None = None, fade_depth: float = 0.9, fade_period: int = 36000,
               lead: int = 6000, tail: int = 6000, offset: int = 0, seed: int = 0, silence: int = 0,
               rate: float = 12000.0) -> np.ndarray:
    """12 ksps float32 audio of an RTTY transmission, the decoder's stand-alone input: continuous
    phase FSK, mark at 915 Hz, space at 915 Hz + `shift`, idle mark for `lead` samples before and
    `tail` after the message.  `text` is a string or the (level, length) runs of baudot_bits.
    `fade` "mark" or "space" lets that tone's amplitude swing between 1 and 1 - `fade_depth`
    every `fade_period` samples; `noise_sigma` adds white noise (counter-based, `seed`); the
    first `offset` samples are dropped, so a stream can start mid-character, and `silence` samples
    of exact zero follow the tail.  Samples are rounded to integers."""
    bits = baudot_bits(text, stopbits) if isinstance(text, str) else text
    line = np.concatenate([np.ones(lead, np.uint8), _rtty_line(bits, baud, rate), np.ones(tail, np.uint8)])
    freq = np.where(line != 0, RTTY_MARK, RTTY_MARK + shift)
    phase = 2.0 * np.pi / rate * np.concatenate([[0.0], np.cumsum(freq)[:-1]])
    gain = np.full(len(line), float(amplitude))
    if fade:
        swing = 1.0 - fade_depth * 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(len(line)) / fade_period))
        gain = np.where((line != 0) == (fade == "mark"), gain * swing, gain)
    s = gain * np.sin(phase)
    if noise_sigma > 0:
        s = s + _noise(np.array([1 << 16 | seed], np.int64), 0, len(line), noise_sigma)[0][0]
    return np.concatenate([np.rint(s)[offset:], np.zeros(silence)]).astype(np.float32)


def rtty_iq(channels, start: int, nframes: int, text: str, shift: float = 170.0, baud: float = 45.45, stopbits: float = 1.5,
            noise_sigma: float = 30.0, carrier: float = 12000.0, amplitude: float = 1500.0, lead: int = 24000,
            fade: str | None = None, fade_depth: float = 0.9, fade_period: int = 144000):
    """48 ksps I/Q of an RTTY signal on the upper side of `carrier`: mark at +915 Hz, space at
    +915 Hz + `shift`, `text` repeated for ever after `lead` frames of idle mark plus a per-channel
    start offset of up to one second; continuous phase, optional fading of the mark or space
    tone, plus noise.  The RTTY text decoder's input through the RX chain (DEMOD_DIGI)."""
    channels = np.asarray(channels, dtype=np.int64)
    ch = channels.astype(np.uint64)
    base = (np.uint64(SEED_BASE) + ch) << np.uint64(20)
    delay = lead + np.floor(FS * _uniform(base + np.uint64(14))).astype(np.int64)
    ph_c = 2.0 * np.pi * _uniform(base + np.uint64(15))
    line = _rtty_line(baudot_bits(text, stopbits, close=True), baud, FS)
    period = len(line)
    spaces = np.concatenate([[0], np.cumsum(line == 0)]).astype(np.int64)     # space frames before frame k of a pass
    n = np.arange(start, start + nframes, dtype=np.int64)
    i_sig = np.empty((len(channels), nframes))
    q_sig = np.empty((len(channels), nframes))
    for k in range(len(channels)):
        rel = n - int(delay[k])
        on = rel >= 0
        r = np.where(on, rel, 0)
        nspace = np.where(on, (r // period) * spaces[period] + spaces[r % period], 0)
        mark = np.where(on, line[r % period] != 0, True)
        ph = 2.0 * np.pi / FS * ((carrier + RTTY_MARK) * n.astype(np.float64) + shift * nspace.astype(np.float64)) + ph_c[k]
        gain = np.full(nframes, float(amplitude))
        if fade:
            swing = 1.0 - fade_depth * 0.5 * (1.0 - np.cos(2.0 * np.pi * n / fade_period))
            gain = np.where(mark == (fade == "mark"), gain * swing, gain)
        i_sig[k], q_sig[k] = gain * np.cos(ph), gain * np.sin(ph)
    if noise_sigma > 0:
        ni, nq = _noise(channels, start, nframes, noise_sigma)
        i_sig, q_sig = i_sig + ni, q_sig + nq
    return _frames(i_sig, q_sig)


def rtty_fixture(path: str) -> dict:
    """A recorded stand-alone RTTY case (an npz of tools/rtty/make_rtty_golden.py) with its input
    regenerated from the recorded arguments and checked against the recorded crc32: the file's
    arrays plus `audio` (float32, read-only) and `config` (shift, speed, stop bits, atc_disable)."""
    import json
    import zlib
    z = np.load(path)
    g = {k: z[k] for k in z.files}
    text = (g["bits_level"], g["bits_length"]) if len(g["bits_level"]) else str(g["message"])
    audio = rtty_audio(text, **json.loads(str(g["gen"])))
    if len(audio) != int(g["samples"]) or zlib.crc32(audio.tobytes()) != int(g["crc32"]):
        raise ValueError(f"{path}: regenerated input differs from the recorded one")
    audio.setflags(write=False)
    g["audio"] = audio
    g["config"] = (int(g["shift_idx"]), int(g["speed_idx"]), int(g["stopbits_idx"]), int(g["atc_disable"]))
    return g


def rtty_chain_fixture(path: str) -> dict:
    """A recorded RTTY case through the receive chain (rtty_chain_*.npz): the file's arrays plus
    `iq` (int32 [frames][2], one channel, read-only) regenerated from the recorded arguments of
    rtty_iq and checked against the recorded crc32, and `config` as above."""
    import json
    import zlib
    z = np.load(path)
    g = {k: z[k] for k in z.files}
    gen = json.loads(str(g["gen"]))
    iq = np.ascontiguousarray(rtty_iq([gen.pop("channel")], 0, gen.pop("nframes"), gen.pop("text"), **gen)[0], dtype=np.int32)
    if zlib.crc32(iq.tobytes()) != int(g["crc32"]):
        raise ValueError(f"{path}: regenerated input differs from the recorded one")
    iq.setflags(write=False)
    g["iq"] = iq
    g["config"] = (int(g["shift_idx"]), int(g["speed_idx"]), int(g["stopbits_idx"]), int(g["atc_disable"]))
    return g


# G3PLX varicode as the BPSK decoder reads it: byte -> code, sent highest bit first and followed by
# two 0 bits; a 0 bit is a phase reversal, a 1 bit none.  Codes start and end with a 1 and hold no
# two 0 bits in a row; bytes 128 .. 255 take the valid codes the ASCII half leaves unused, in order.
_VARICODE_ASCII = (
    "2AB 2DB 2ED 377 2EB 35F 2EF 2FD 2FF 0EF 01D 36F 2DD 01F 375 3AB 2F7 2F5 3AD 3AF 35B 36B 36D 357 37B 37D 3B7 355 35D 3BB 2FB 37F "
    "001 1FF 15F 1F5 1DB 2D5 2BB 17F 0FB 0F7 16F 1DF 075 035 057 1AF 0B7 0BD 0ED 0FF 177 15B 16B 1AD 1AB 1B7 0F5 1BD 1ED 055 1D7 2AF "
    "2BD 07D 0EB 0AD 0B5 077 0DB 0FD 155 07F 1FD 17D 0D7 0BB 0DD 0AB 0D5 1DD 0AF 06F 06D 157 1B5 15D 175 17B 2AD 1F7 1EF 1FB 2BF 16D "
    "2DF 00B 05F 02F 02D 003 03D 05B 02B 00D 1EB 0BF 01B 03B 00F 007 03F 1BF 015 017 005 037 07B 06B 0DF 05D 1D5 2B7 1BB 2B5 2D7 3B5")
PSK_SPEEDS = (31.25, 62.5, 125.0)                            # speed_idx 0 .. 2
PSK_CARRIER = 500.0


def varicode_table():
    """code of every byte 0 .. 255"""
    codes = [int(x, 16) for x in _VARICODE_ASCII.split()]
    used, c = set(codes), 0
    while len(codes) < 256:
        c += 1
        b = bin(c)[2:]
        if b[-1] == "1" and "00" not in b and c not in used:
            codes.append(c)
    return codes


def varicode_bits(data, preamble: int = 8, idle_ones: int = 0, postamble: int = 8) -> np.ndarray:
    """The bit stream that sends `data` (bytes or a latin-1 string): `preamble` 0 bits (reversals,
    the idle of a BPSK transmitter), `idle_ones` 1 bits (steady carrier), every byte's code followed
    by two 0 bits, `postamble` 0 bits."""
    if isinstance(data, str):
        data = data.encode("latin-1")
    table = varicode_table()
    bits = [0] * preamble + [1] * idle_ones
    for byte in data:
        bits += [int(b) for b in bin(table[byte])[2:]] + [0, 0]
    return np.array(bits + [0] * postamble, np.uint8)


def _psk_baseband(bits, per_bit: int, first: float = 1.0) -> np.ndarray:
    """The envelope between -1 and 1, len(bits) * per_bit samples from the centre of the bit before
    the first: constant through a 1 bit, half a cosine from one polarity to the other through a 0
    bit (a raised-cosine reversal, centre to centre)."""
    pol = first * np.cumprod(np.concatenate([[1.0], np.where(np.asarray(bits) != 0, 1.0, -1.0)]))
    a, b = np.repeat(pol[:-1], per_bit), np.repeat(pol[1:], per_bit)
    frac = np.tile(np.arange(per_bit) / per_bit, len(bits))
    return 0.5 * (a + b) + 0.5 * (a - b) * np.cos(np.pi * frac)


def psk_audio(text, baud: float = 31.25, amplitude: float = 1000.0, offset: int = 0, noise_sigma: float = 0.0, df: float = 0.0,
              seed: int = 0, preamble: int = 8, idle_ones: int = 0, postamble: int = 8, lead: int = 0, silence: int = 0,
              repeat: int = 1, rate: float = 12000.0) -> np.ndarray:
    """12 ksps float32 audio of a BPSK transmission, the decoder's stand-alone input: a carrier at
    500 Hz + `df` whose polarity follows varicode_bits(text, preamble, idle_ones, postamble) with
    raised-cosine reversals, after `lead` samples of steady carrier.  `noise_sigma` adds white noise
    (counter-based, `seed`); the first `offset` samples are dropped, which moves the bit boundaries
    against the decoder's fixed symbol clock and lets a stream start mid-character.  `silence`
    samples of exact zero follow, and the whole is sent `repeat` times.
    Samples are not rounded: amplitudes from 1e-28 to 1e34 are meaningful inputs."""
    per_bit = int(round(rate / baud))
    m = np.concatenate([np.ones(lead), _psk_baseband(varicode_bits(text, preamble, idle_ones, postamble), per_bit)])
    s = amplitude * m * np.sin(2.0 * np.pi * (PSK_CARRIER + df) / rate * np.arange(len(m)))
    if noise_sigma > 0:
        s = s + _noise(np.array([2 << 16 | seed], np.int64), 0, len(m), noise_sigma)[0][0]
    with np.errstate(over="ignore"):
        return np.tile(np.concatenate([s[offset:], np.zeros(silence)]), repeat).astype(np.float32)


def psk_iq(channels, start: int, nframes: int, text: str, baud: float = 31.25, noise_sigma: float = 30.0, carrier: float = 12000.0,
           amplitude: float = 1500.0, lead: int = 24000, df: float = 0.0, preamble: int = 16):
    """48 ksps I/Q of a BPSK signal on the upper side of `carrier`, at +500 Hz + `df`: steady carrier
    for `lead` frames plus a per-channel start offset of up to one second, then `preamble` reversals
    and `text`, repeated for ever; plus noise.  The BPSK text decoder's input through the RX chain
    (DEMOD_DIGI)."""
    channels = np.asarray(channels, dtype=np.int64)
    ch = channels.astype(np.uint64)
    base = (np.uint64(SEED_BASE) + ch) << np.uint64(20)
    delay = lead + np.floor(FS * _uniform(base + np.uint64(16))).astype(np.int64)
    ph_c = 2.0 * np.pi * _uniform(base + np.uint64(17))
    bits = varicode_bits(text, preamble, 0, 0)
    env = _psk_baseband(np.concatenate([bits, bits]), int(round(FS / baud)))      # two passes: an even number of reversals
    n = np.arange(start, start + nframes, dtype=np.int64)
    i_sig = np.empty((len(channels), nframes))
    q_sig = np.empty((len(channels), nframes))
    for k in range(len(channels)):
        rel = n - int(delay[k])
        m = np.where(rel >= 0, env[np.where(rel >= 0, rel, 0) % len(env)], 1.0)
        ph = 2.0 * np.pi / FS * (carrier + PSK_CARRIER + df) * n.astype(np.float64) + ph_c[k]
        i_sig[k], q_sig[k] = amplitude * m * np.cos(ph), amplitude * m * np.sin(ph)
    if noise_sigma > 0:
        ni, nq = _noise(channels, start, nframes, noise_sigma)
        i_sig, q_sig = i_sig + ni, q_sig + nq
    return _frames(i_sig, q_sig)


def psk_fixture(path: str) -> dict:
    """A recorded stand-alone BPSK case (an npz of tools/psk/make_psk_golden.py) with its input
    regenerated from the recorded arguments and checked against the recorded crc32: the file's
    arrays plus `audio` (float32, read-only), `sent` (bytes) and `speed` (speed_idx)."""
    import json
    import zlib
    z = np.load(path)
    g = {k: z[k] for k in z.files}
    g["sent"] = bytes(g["message"])
    audio = psk_audio(g["sent"], **json.loads(str(g["gen"])))
    if len(audio) != int(g["samples"]) or zlib.crc32(audio.tobytes()) != int(g["crc32"]):
        raise ValueError(f"{path}: regenerated input differs from the recorded one")
    audio.setflags(write=False)
    g["audio"] = audio
    g["speed"] = int(g["speed_idx"])
    return g


def psk_chain_fixture(path: str) -> dict:
    """A recorded BPSK case through the receive chain (psk_chain_*.npz): the file's arrays plus `iq`
    (int32 [frames][2], one channel, read-only) regenerated from the recorded arguments of psk_iq
    and checked against the recorded crc32, and `speed`."""
    import json
    import zlib
    z = np.load(path)
    g = {k: z[k] for k in z.files}
    gen = json.loads(str(g["gen"]))
    iq = np.ascontiguousarray(psk_iq([gen.pop("channel")], 0, gen.pop("nframes"), gen.pop("text"), **gen)[0], dtype=np.int32)
    if zlib.crc32(iq.tobytes()) != int(g["crc32"]):
        raise ValueError(f"{path}: regenerated input differs from the recorded one")
    iq.setflags(write=False)
    g["iq"] = iq
    g["speed"] = int(g["speed_idx"])
    return g


def nr_audio(nsamples: int, rate: float = 6000.0, snr_db: float = 10.0, seed: int = 0, amplitude: float = 3000.0,
             f0: float = 130.0, tone: float = 700.0, floor: float = 1.0, segment: float = 0.4) -> np.ndarray:
    """float32 audio at the noise reduction's input (post-AGC amplitude), `rate` 6000 or 12000: a
    repeating sequence of four segments of `segment` seconds -- a voiced signal (harmonics of `f0` up
    to 2.4 kHz falling with 1 / k under a 5 Hz syllable envelope), a gap, a keyed CW `tone`
    (60 ms dots), a gap -- plus white noise (counter-based, `seed`) `snr_db` below the voiced
    signal's RMS.  In the gaps only the noise and a constant noise floor of `floor` sigma remain."""
    t = np.arange(nsamples) / rate
    seg = np.floor(t / segment).astype(np.int64) % 4
    k = np.arange(1, int(2400.0 / f0) + 1)
    voiced = (np.sin(2.0 * np.pi * f0 * t[:, None] * k[None, :]) / k[None, :]).sum(axis=1)
    voiced *= 0.5 - 0.5 * np.cos(2.0 * np.pi * 5.0 * t)
    cw = np.sin(2.0 * np.pi * tone * t) * (np.floor(t / 0.06).astype(np.int64) % 2 == 0)
    rms = np.sqrt(np.mean(voiced ** 2)) if nsamples else 1.0
    s = amplitude * (np.where(seg == 0, voiced / max(rms, 1e-12), 0.0) + np.where(seg == 2, cw, 0.0))
    sigma = amplitude * 10.0 ** (-snr_db / 20.0)
    ni, nq = _noise(np.array([3 << 16 | seed], np.int64), 0, nsamples, 1.0)
    return (s + sigma * ni[0] + floor * nq[0]).astype(np.float32)


def nr_fixture(path: str) -> dict:
    """A recorded noise-reduction case (an npz of tools/nr/make_nr_golden.py) with its input
    regenerated from the recorded arguments of nr_audio and checked against the recorded crc32: the
    file's arrays plus `audio` (float32, read-only) and `cfg` (the configuration as a dict)."""
    import json
    import zlib
    z = np.load(path)
    g = {k: z[k] for k in z.files}
    audio = nr_audio(**json.loads(str(g["gen"])))
    if len(audio) != int(g["samples"]) or zlib.crc32(audio.tobytes()) != int(g["crc32"]):
        raise ValueError(f"{path}: regenerated input differs from the recorded one")
    audio.setflags(write=False)
    g["audio"] = audio
    g["cfg"] = json.loads(str(g["config"]))
    return g


def nb_audio(nsamples: int, seed: int = 0, kind: str = "voiced", sigma: float = 300.0, a1: float = 1.6, a2: float = -0.8,
             impulses=(), scale: float = 1.0, tone: float = 1000.0, rate: float = 12000.0, amplitude: float = 3000.0,
             nan_at: int = -1, inf_at: int = -1, ramp: int = 0) -> np.ndarray:
    """float32 audio at the noise blanker's input.  `kind`: "voiced", a low-order resonator
    y[i] = a1 y[i-1] + a2 y[i-2] + e driven by white noise e of `sigma` (counter-based, `seed`);
    "tone", a sine of `tone` Hz and `amplitude` plus that noise; "noise", the noise alone; "dc",
    `amplitude` everywhere; "silence".  `impulses`: (position, amplitude) pairs added on top, one
    sample each.  The first `ramp` samples fade in under a raised cosine.  The sum is multiplied by
    `scale` in double and rounded to float32; then the sample at `nan_at` becomes a NaN and the one at
    `inf_at` an infinity."""
    e = sigma * _noise(np.array([4 << 16 | seed], np.int64), 0, nsamples, 1.0)[0][0]
    if kind == "voiced":
        y = np.zeros(nsamples)
        y1 = y2 = 0.0
        for i in range(nsamples):
            y[i] = a1 * y1 + a2 * y2 + e[i]
            y2, y1 = y1, y[i]
    elif kind == "tone":
        y = amplitude * np.sin(2.0 * np.pi * tone * np.arange(nsamples) / rate) + e
    elif kind == "noise":
        y = e.copy()
    elif kind == "dc":
        y = np.full(nsamples, float(amplitude))
    elif kind == "silence":
        y = np.zeros(nsamples)
    else:
        raise ValueError(f"nb_audio: kind {kind!r}")
    for pos, amp in impulses:
        y[int(pos)] += float(amp)
    if ramp > 0:
        y[:ramp] *= 0.5 - 0.5 * np.cos(np.pi * np.arange(min(ramp, nsamples)) / ramp)
    x = (y * scale).astype(np.float32)
    if nan_at >= 0:
        x[nan_at] = np.float32("nan")
    if inf_at >= 0:
        x[inf_at] = np.float32("inf")
    return x


def nb_fixture(path: str) -> dict:
    """A recorded noise-blanker case (an npz of tools/nb/make_nb_golden.py) with its input regenerated
    from the recorded arguments of nb_audio and checked against the recorded crc32: the file's arrays
    plus `audio` (float32, read-only) and `cfg` (the settings as a dict)."""
    import json
    import zlib
    z = np.load(path)
    g = {k: z[k] for k in z.files}
    audio = nb_audio(**json.loads(str(g["gen"])))
    if len(audio) != int(g["samples"]) or zlib.crc32(audio.tobytes()) != int(g["crc32"]):
        raise ValueError(f"{path}: regenerated input differs from the recorded one")
    audio.setflags(write=False)
    g["audio"] = audio
    g["cfg"] = json.loads(str(g["config"]))
    return g
