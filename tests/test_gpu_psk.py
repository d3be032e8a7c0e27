"""BPSK decoder on the device (psk_decode, uhsdr_psk.hip): the stand-alone decoder against the
reference firmware's recorded output (tests/golden/psk_*.npz) with a different case on each lane,
and against the host build of the same step functions on arbitrary input.  Everything is compared
exactly.  The call sizes aim at the edges of the kernel's 32-sample LDS tiles and of the 24-entry
product ring, of which a short call moves only the slots it touches: 1, 8, 23, 25 and 33 samples,
lengths that are no multiple of the tile, rows longer than the call, a partial last wave.

Then the decoder inside the receive chain (uhsdr_rx_set_psk_text) against the bytes the reference
chain printed (psk_chain_*.npz) and against the host decoder on the chain's own tap."""
import ctypes as C
import zlib

import numpy as np
import pytest

import uhsdr_amd as U
from psk_cases import CASES, load_case, load_chain_case
from uhsdr_amd import psk, synth

pytestmark = pytest.mark.gpu

ODD = (1, 23, 25, 33, 97, 8, 24, 32, 64, 7)      # call sizes around the ring of 24 and the tile of 32


def group(speed, skip=("chartable125",)):
    return [g for g in (load_case(n) for n in CASES) if g["speed"] == speed and g["name"] not in skip]


class Tiled:
    """cases of one speed over channels, channel c running case (c + shift) % n; rows padded with
    zeros to the longest case plus `pad`, every channel checked up to its own case's length"""

    def __init__(self, cases, channels, shift=0, pad=0, limit=None):
        self.g = [cases[(c + shift) % len(cases)] for c in range(channels)]
        self.len = np.array([min(len(g["audio"]), limit or len(g["audio"])) for g in self.g])
        self.samples = int(self.len.max())
        self.stride = self.samples + pad
        self.rows = np.zeros((channels, self.stride), np.float32)
        for c, g in enumerate(self.g):
            self.rows[c, :self.len[c]] = g["audio"][:self.len[c]]

    def check(self, done, text, total, cap):
        """after `done` samples: the characters whose sample lies before, for every case that reaches so far"""
        for c in np.flatnonzero(self.len >= done):
            g = self.g[c]
            n = int(np.searchsorted(g["char_sample"], done, "left"))
            assert int(total[c]) == n, (c, g["name"], done)
            k = np.arange(max(0, n - cap), n)
            assert bytes(text[c, k % cap]) == bytes(g["chars"][k]), (c, g["name"], done)


def bounds_of(sizes, samples):
    out, at, i = [], 0, 0
    while at < samples:
        at = min(at + sizes[i % len(sizes)], samples)
        out.append(at)
        i += 1
    return out


def feed(t, dec, bounds, cap, check_every=1):
    """calls from bound to bound on rows of the whole stream's stride (stride > n), read back at some"""
    import torch
    lib = U.load()
    rows = torch.from_numpy(t.rows).cuda()
    last = 0
    for i, b in enumerate(bounds):
        st = lib.uhsdr_psk_process(dec.handle, C.c_void_p(rows.data_ptr() + 4 * last), b - last, t.stride)
        assert st == 0, lib.uhsdr_last_error()
        if i % check_every == 0 or b == bounds[-1]:
            text, total = dec.read()
            t.check(b, text, total, cap)
        last = b
    dec.synchronize()


@pytest.mark.parametrize("channels,cap", [(1, 64), (63, 8), (65, 64), (130, 8)])
def test_fixtures_tiled_over_lanes_whole_streams(cuda, channels, cap):
    t = Tiled(group(2), channels, shift=channels)
    assert channels == 1 or len({int(x) % 32 for x in t.len}) > 2       # tile remainders
    dec = psk.PskDecoder(channels, 2, capacity=cap)
    feed(t, dec, sorted(set(int(x) for x in t.len)), cap)      # one piece up to each case's end
    assert int(dec.read()[1].max()) > 8                        # the ring of capacity 8 wrapped
    dec.close()


@pytest.mark.parametrize("channels,cap", [(1, 8), (63, 64), (65, 8), (130, 64)])
def test_fixtures_tiled_over_lanes_isr_sized_calls(cuda, channels, cap):
    """8 samples per call, what one 32-frame block of the firmware's interrupt delivers"""
    t = Tiled(group(2), channels, shift=channels, limit=16000)
    dec = psk.PskDecoder(channels, 2, capacity=cap)
    feed(t, dec, bounds_of((8,), t.samples), cap, check_every=500)
    dec.close()


@pytest.mark.parametrize("channels,cap", [(1, 64), (63, 8), (65, 64), (130, 8)])
def test_fixtures_tiled_over_lanes_odd_calls(cuda, channels, cap):
    """calls of 1, 23, 25, 33, 97 ... samples in turn, on rows far longer than the call"""
    t = Tiled(group(2), channels, shift=channels, pad=61, limit=30000)
    dec = psk.PskDecoder(channels, 2, capacity=cap)
    feed(t, dec, bounds_of(ODD, t.samples), cap, check_every=100)
    dec.close()


def test_denormal_burst_and_clean_rows_side_by_side(cuda):
    """the 1e-26 stream, whose symbol product is denormal, the stream that decays into denormals
    through 60,000 zeros, and a clean one, in the lanes of one wave"""
    cases = [load_case(n) for n in ("tiny", "burst", "clean125")]
    t = Tiled(cases, 64)
    dec = psk.PskDecoder(64, 2, capacity=128)
    feed(t, dec, bounds_of((1000, 333), t.samples), 128, check_every=40)
    text, total = dec.read()
    # (feed checked every row up to its own case's end; the longest, the burst, ends the stream)
    assert len(cases[0]["chars"]) > 30 and bytes(text[1, :int(total[1])]).count(cases[1]["sent"]) == 2
    dec.close()


@pytest.mark.parametrize("speed", [0, 1, 2])
def test_every_speed(cuda, speed):
    cases = group(speed, skip=()) if speed == 2 else group(speed)
    if speed == 2:
        cases = [g for g in cases if g["name"] in ("chartable125", "clean125", "idle60")]
    t = Tiled(cases, 65, pad=3)
    dec = psk.PskDecoder(65, speed, capacity=512)
    feed(t, dec, sorted(set(int(x) for x in t.len)), 512)
    dec.close()


def arbitrary_input(channels, samples, seed):
    """fragments of BPSK at arbitrary offsets, levels and small carrier errors plus seeded noise,
    stretches of exact zeros (the filter runs down into denormals), a 1e-26 row and a few wild
    samples"""
    rng = np.random.default_rng(seed)
    x = np.zeros((channels, samples), np.float32)
    for c in range(channels):
        frag = synth.psk_audio("de UHSDR 599 73 k " * 3, baud=125.0, amplitude=200.0 + 37.0 * c, df=0.02 * (c % 7), preamble=4)
        off = int(rng.integers(0, 2000))
        n = min(len(frag) - off, samples)
        x[c, :n] = frag[off:off + n]
        x[c] += (rng.standard_normal(samples) * (5.0 + 11.0 * (c % 9))).astype(np.float32)
        if c % 4 == 1:
            x[c, 15000:21000] = 0.0
    x[7, 9000] = np.inf
    x[8, 9000:9003] = np.nan
    x[9, 5000:5100] = 3.0e38
    x[10] = synth.psk_audio("de UHSDR 599 73 k " * 3, baud=125.0, amplitude=1e-26)[:samples]
    return x


def same_floats(a, b):
    """bit for bit; a NaN equals a NaN, since IEEE 754 leaves the sign and payload of a NaN that an
    operation makes to the processor, and the host's and the device's differ"""
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def same(got, want):
    return all(same_floats(a, b) if a.dtype == np.float32 else np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("speed,per_call", [(2, 24000), (2, 1000), (2, 333), (1, 25)])
def test_device_equals_host_on_arbitrary_input(cuda, speed, per_call):
    import torch
    samples = 24000
    x = arbitrary_input(130, samples, 20261020)
    host = psk.PskDecoder(130, speed, capacity=64, host=True)
    host.process(x)
    want = host.read() + (host.symbol(),)
    if speed == 2:
        assert int(np.count_nonzero(want[1] >= 4)) > 100           # text on most channels, or the test shows nothing
        assert int(want[1][10]) >= 4                               # the 1e-26 row among them
    assert np.count_nonzero(want[2]) > 120 and not np.isfinite(want[2][7:10]).any()
    dec = psk.PskDecoder(130, speed, capacity=64)
    d = torch.from_numpy(x).cuda()
    for b in range(0, samples, per_call):
        dec.process(d[:, b:b + per_call].contiguous())
    assert same(dec.read() + (dec.symbol(),), want)
    dec.reset()
    dec.process(d)
    assert same(dec.read() + (dec.symbol(),), want)
    assert dec.new_text() == host.new_text()
    dec.close()
    host.close()


def test_device_argument_errors(cuda):
    import torch
    lib = U.load()
    dec = psk.PskDecoder(4, 2, capacity=8)
    x = torch.zeros((4, 16), dtype=torch.float32, device="cuda")
    assert lib.uhsdr_psk_process(dec.handle, C.c_void_p(x.data_ptr()), 17, 16) == -2
    assert lib.uhsdr_psk_process(dec.handle, C.c_void_p(x.data_ptr()), -1, 16) == -2
    assert lib.uhsdr_psk_process(dec.handle, None, 4, 16) == -1
    assert lib.uhsdr_psk_process_host(dec.handle, C.c_void_p(x.data_ptr()), 4, 16) == -1      # a device handle
    assert lib.uhsdr_psk_process(dec.handle, C.c_void_p(x.data_ptr()), 0, 16) == 0
    dec.process(x)
    assert int(dec.read()[1].sum()) == 0 and not dec.symbol().any()
    dec.close()


# ---- through the RX chain ----

RX_C = 65                   # a full wave and a partial one; every channel gets the recorded channel's I/Q
FAST, SLOW = "chain_p48_125", "chain_p48_31"
_rx = {}


def rx_config(g, **kw):
    return U.default_config(**dict(dict(filter_path=int(g["path"]), dmod_mode=U.DEMOD_DIGI), **kw))


def rx_input(name):
    """the fixture and its I/Q on the device, [RX_C][frames][2]"""
    import torch
    if name not in _rx:
        g = load_chain_case(name)
        _rx[name] = (g, torch.from_numpy(g["iq"].copy()).cuda().unsqueeze(0).expand(RX_C, -1, -1))
    return _rx[name]


def check_tap(g, tap):
    """tap [RX_C][N/4] of the whole stream: every lane the reference's samples"""
    assert np.array_equal(tap.view(np.uint32), np.broadcast_to(tap[:1].view(np.uint32), tap.shape))
    for c in (0, RX_C - 1):
        crc = np.array([zlib.crc32(tap[c, k:k + 8].tobytes()) for k in range(0, tap.shape[1], 8)], dtype=np.uint32)
        bad = np.flatnonzero(crc != g["tap_crc"])
        assert len(bad) == 0, (c, len(bad), bad[:8])
        assert np.array_equal(tap[c, :256].view(np.uint32), g["tap_head"].view(np.uint32))


def check_text(g, text, total):
    want = g["chars"]
    assert str(g["message"]).encode() in bytes(want)
    assert np.array_equal(total, np.full(RX_C, len(want), np.uint32))
    assert np.array_equal(text[:, :len(want)], np.broadcast_to(want, (RX_C, len(want))))


@pytest.mark.parametrize("frames", [256, 2048])
def test_text_through_the_rx_chain(cuda, back, frames):
    """the text is the reference's and the host decoder's on the chain's own tap, the tap is the
    reference's.  256-frame calls: the decoder reads the caller's tap row; 2048: the handle's own
    row, and the tap comes from a second chain without text, whose audio must be the same."""
    import torch
    g, iq = rx_input(FAST)
    cap = 256
    off_chain = U.RxChain(rx_config(g), channels=RX_C, frames=frames)
    on_chain = U.RxChain(rx_config(g), channels=RX_C, frames=frames)
    tap = torch.zeros((RX_C, frames // 4), dtype=torch.float32, device="cuda")
    (on_chain if frames == 256 else off_chain).set_digi_tap(tap)
    on_chain.set_psk_text(True, g["speed"], text_capacity=cap)
    audio = [torch.empty((RX_C, frames), dtype=torch.float32, device="cuda") for _ in range(2)]
    dst = [torch.empty((RX_C, frames, 2), dtype=torch.int32, device="cuda") for _ in range(2)]
    rows, pieces = [], [b""] * RX_C
    for k in range(iq.shape[1] // frames):
        x = iq[:, k * frames:(k + 1) * frames].contiguous()
        off_chain.process(x, audio[0], dst[0])
        on_chain.process(x, audio[1], dst[1])
        torch.cuda.synchronize()
        assert torch.equal(audio[0].view(torch.int32), audio[1].view(torch.int32)), k
        assert torch.equal(dst[0], dst[1]), k
        rows.append(tap.clone())
        if k % 37 == 0:
            pieces = [a + b for a, b in zip(pieces, on_chain.psk_text())]
    pieces = [a + b for a, b in zip(pieces, on_chain.psk_text())]
    text, total = on_chain.psk_text_outputs.read()
    symbol = on_chain.psk_text_outputs.read_symbol()
    rows = torch.cat(rows, dim=1).cpu().numpy()
    check_tap(g, rows)
    host = psk.PskDecoder(RX_C, g["speed"], capacity=cap, host=True)
    host.process(np.ascontiguousarray(rows))
    htext, htotal = host.read()
    assert np.array_equal(total, htotal) and np.array_equal(text, htext)
    assert np.array_equal(symbol.view(np.uint32), host.symbol().view(np.uint32))
    check_text(g, text, total)
    assert pieces == [bytes(g["chars"])] * RX_C
    for ch in (off_chain, on_chain, host):
        ch.close()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_rx_pipelined_modes_give_the_serial_text(cuda, mode):
    """the decode launch follows the kernel that wrote the tap row on the side stream: calls enqueued
    back to back, no synchronisation between them (mode 3 runs as 2 with the tap on)"""
    g, iq = rx_input(FAST)
    frames = 256
    xs = [iq[:, k * frames:(k + 1) * frames].contiguous() for k in range(iq.shape[1] // frames)]
    out = []
    for m in (0, mode):
        chain = U.RxChain(rx_config(g), channels=RX_C, frames=frames)
        chain.set_pipelined(m)
        chain.set_psk_text(True, g["speed"], text_capacity=256)
        for x in xs:
            chain.process(x)
        chain.join()
        chain.synchronize()
        out.append(chain.psk_text_outputs.read() + (chain.psk_text_outputs.read_symbol().view(np.uint32),))
        chain.close()
    check_text(g, *out[0][:2])
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_rx_reset_restarts_the_decoder(cuda, back):
    """BPSK31 at 2048 frames per call, twice with a reset between"""
    g, iq = rx_input(SLOW)
    frames = 2048
    chain = U.RxChain(rx_config(g), channels=RX_C, frames=frames)
    chain.set_psk_text(True, g["speed"], text_capacity=256)
    runs = []
    for _ in range(2):
        for k in range(iq.shape[1] // frames):
            chain.process(iq[:, k * frames:(k + 1) * frames].contiguous())
        chain.synchronize()
        runs.append((chain.psk_text_outputs.read(), chain.psk_text()))
        chain.reset()
    check_text(g, *runs[0][0])
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a, b)
    assert runs[0][1] == runs[1][1]
    chain.close()


def test_rx_text_only_where_the_firmware_decodes(cuda):
    refused = (dict(dmod_mode=U.DEMOD_USB, filter_path=48), dict(dmod_mode=U.DEMOD_SAM, filter_path=70),
               dict(dmod_mode=U.DEMOD_FM, filter_path=1), dict(dmod_mode=U.DEMOD_DIGI, filter_path=60))     # P60: 24 ksps
    for kw in refused:
        chain = U.RxChain(U.default_config(**kw), channels=4, frames=256)
        with pytest.raises(U.UhsdrError) as e:
            chain.set_psk_text(True, 0, text_capacity=64)
        assert e.value.status == U.UHSDR_ARGUMENT_ERROR and "psk text" in str(e.value)
        chain.close()
    chain = U.RxChain(U.default_config(dmod_mode=U.DEMOD_DIGI, filter_path=48), channels=4, frames=256)
    for bad in ((3, 64), (-1, 64), (0, 4)):
        with pytest.raises(U.UhsdrError) as e:
            chain.set_psk_text(True, *bad)
        assert e.value.status == U.UHSDR_ARGUMENT_ERROR
    with pytest.raises(RuntimeError):
        chain.psk_text()
    # the firmware's digital_mode is one value: one text decoder at a time
    chain.set_rtty_text(True, 1, 0, 1, False, text_capacity=8)
    with pytest.raises(U.UhsdrError) as e:
        chain.set_psk_text(True, 2, text_capacity=8)
    assert e.value.status == U.UHSDR_ARGUMENT_ERROR and "rtty text is on" in str(e.value)
    chain.set_psk_text(False)                      # turning off what is off is no error and leaves RTTY text on
    assert chain.rtty_text() == [b""] * 4
    chain.set_rtty_text(False)
    chain.set_psk_text(True, 2, text_capacity=8)
    with pytest.raises(U.UhsdrError) as e:
        chain.set_rtty_text(True, 1, 0, 1, False, text_capacity=8)
    assert e.value.status == U.UHSDR_ARGUMENT_ERROR and "psk text is on" in str(e.value)
    assert chain.psk_text() == [b""] * 4
    chain.set_psk_text(False)
    chain.set_rtty_text(True, 1, 0, 1, False, text_capacity=8)
    chain.set_rtty_text(False)
    chain.close()
