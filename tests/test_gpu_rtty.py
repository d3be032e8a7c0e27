"""RTTY decoder on the device (rtty_decode, uhsdr_rtty.hip): the stand-alone decoder against the
reference firmware's recorded output (tests/golden/rtty_*.npz) with a different case on each lane,
and against the host build of the same step function on arbitrary input.  Everything is compared
exactly.  The call sizes aim at the edges of the kernel's 32-sample LDS tiles: lengths that are no
multiple of the tile, calls shorter than a tile, rows longer than the call, a partial last wave.

Then the decoder inside the receive chain: the digital-mode tap (uhsdr_rx_set_digi_tap) against the
samples the reference chain handed its demodulator (rtty_chain_*.npz: a crc32 per 32-frame call and
the first 256 samples), in every schedule, and the text of uhsdr_rx_set_rtty_text against the host
decoder on that tap and against the bytes the reference printed."""
import ctypes as C
import zlib

import numpy as np
import pytest

import uhsdr_amd as U
from rtty_cases import CASES, CHAIN_CASES, load_case, load_chain_case
from uhsdr_amd import rtty, synth

pytestmark = pytest.mark.gpu

MAIN = (1, 0, 1, 0)        # 170 Hz, 45.45 baud, 1.5 stop bits, ATC on: the configuration most cases share


def group(config):
    return [g for g in (load_case(n) for n in CASES) if g["config"] == config]


class Tiled:
    """cases of one configuration over channels, channel c running case (c + shift) % n; rows padded
    with zeros to the longest case plus `pad`, every channel checked up to its own case's length"""

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
            assert int(total[c]) == n, (c, done)
            k = np.arange(max(0, n - cap), n)
            assert bytes(text[c, k % cap]) == bytes(g["chars"][k]), (c, done)


def feed(t, dec, bounds, cap, check_every=1):
    """calls from bound to bound on rows of the whole stream's stride (stride > n), read back at some"""
    import torch
    lib = U.load()
    rows = torch.from_numpy(t.rows).cuda()
    last = 0
    for i, b in enumerate(bounds):
        st = lib.uhsdr_rtty_process(dec.handle, C.c_void_p(rows.data_ptr() + 4 * last), b - last, t.stride)
        assert st == 0, lib.uhsdr_last_error()
        if i % check_every == 0 or b == bounds[-1]:
            text, total = dec.read()
            t.check(b, text, total, cap)
        last = b
    dec.synchronize()


@pytest.mark.parametrize("channels,cap", [(1, 64), (63, 8), (65, 64), (130, 8)])
def test_fixtures_tiled_over_lanes_whole_streams(cuda, channels, cap):
    t = Tiled(group(MAIN), channels, shift=channels)
    assert t.samples % 32 != 0 and (channels == 1 or len({int(x) % 32 for x in t.len}) > 2)       # tile remainders
    dec = rtty.RttyDecoder(channels, *MAIN, capacity=cap)
    feed(t, dec, sorted(set(int(x) for x in t.len)), cap)      # one piece up to each case's end
    assert int(dec.read()[1].max()) > 8                        # the ring of capacity 8 wrapped
    dec.close()


@pytest.mark.parametrize("channels,cap", [(1, 8), (63, 64), (65, 8), (130, 64)])
def test_fixtures_tiled_over_lanes_isr_sized_calls(cuda, channels, cap):
    """8 samples per call, what one 32-frame block of the firmware's interrupt delivers"""
    t = Tiled(group(MAIN), channels, shift=channels, limit=24000)
    dec = rtty.RttyDecoder(channels, *MAIN, capacity=cap)
    feed(t, dec, list(range(8, t.samples, 8)) + [t.samples], cap, check_every=500)
    dec.close()


@pytest.mark.parametrize("channels,cap", [(1, 64), (63, 8), (65, 64), (130, 8)])
def test_fixtures_tiled_over_lanes_odd_calls(cuda, channels, cap):
    """97 samples per call, three tiles and one sample, on rows far longer than the call"""
    t = Tiled(group(MAIN), channels, shift=channels, pad=61, limit=70000)
    dec = rtty.RttyDecoder(channels, *MAIN, capacity=cap)
    feed(t, dec, list(range(97, t.samples, 97)) + [t.samples], cap, check_every=100)
    dec.close()


def test_every_configuration(cuda):
    configs = sorted({load_case(n)["config"] for n in CASES} - {MAIN})
    assert len(configs) >= 10
    for cfg in configs:
        t = Tiled(group(cfg), 65, pad=3)
        dec = rtty.RttyDecoder(65, *cfg, capacity=16)
        feed(t, dec, sorted(set(int(x) for x in t.len)), 16)
        dec.close()


def arbitrary_input(channels, samples, seed):
    """seeded noise of a different level per channel plus fragments of FSK at arbitrary offsets, a
    stretch of exact zeros (the filters run down into denormals) and a few wild samples"""
    rng = np.random.default_rng(seed)
    x = np.zeros((channels, samples), np.float32)
    for c in range(channels):
        frag = synth.rtty_audio("RYRY UHSDR 599 " * 3, shift=170.0, baud=45.45, stopbits=1.0 + 0.5 * (c % 3),
                                amplitude=200.0 + 37.0 * c, lead=500 + 13 * c, tail=0)
        off = int(rng.integers(0, 4000))
        n = min(len(frag) - off, samples)
        x[c, :n] = frag[off:off + n]
        x[c] += (rng.standard_normal(samples) * (5.0 + 11.0 * (c % 9))).astype(np.float32)
        if c % 4 == 1:
            x[c, 15000:21000] = 0.0
    x[7, 9000] = np.inf
    x[8, 9000:9003] = np.nan
    x[9, 5000:5100] = 3.0e38
    return x


@pytest.mark.parametrize("config,per_call", [(MAIN, 24000), (MAIN, 1000), ((1, 0, 0, 1), 333)])
def test_device_equals_host_on_arbitrary_input(cuda, config, per_call):
    import torch
    x = arbitrary_input(130, 24000, 20261020)
    host = rtty.RttyDecoder(130, *config, capacity=64, host=True)
    host.process(x)
    want = host.read()
    assert int(np.count_nonzero(want[1] >= 4)) > 100           # text on most channels, or the test shows nothing
    dec = rtty.RttyDecoder(130, *config, capacity=64)
    d = torch.from_numpy(x).cuda()
    for b in range(0, 24000, per_call):
        dec.process(d[:, b:b + per_call].contiguous())
    for got, ref in zip(dec.read(), want):
        assert np.array_equal(got, ref)
    dec.reset()
    dec.process(d)
    for got, ref in zip(dec.read(), want):
        assert np.array_equal(got, ref)
    assert dec.new_text() == host.new_text()
    dec.close()
    host.close()


def test_device_argument_errors(cuda):
    import torch
    lib = U.load()
    dec = rtty.RttyDecoder(4, *MAIN, capacity=8)
    x = torch.zeros((4, 16), dtype=torch.float32, device="cuda")
    assert lib.uhsdr_rtty_process(dec.handle, C.c_void_p(x.data_ptr()), 17, 16) == -2
    assert lib.uhsdr_rtty_process(dec.handle, None, 4, 16) == -1
    assert lib.uhsdr_rtty_process_host(dec.handle, C.c_void_p(x.data_ptr()), 4, 16) == -1      # a device handle
    assert lib.uhsdr_rtty_process(dec.handle, C.c_void_p(x.data_ptr()), 0, 16) == 0
    dec.process(x)
    assert int(dec.read()[1].sum()) == 0
    dec.close()


# ---- through the RX chain ----

RX_C = 65                   # a full wave and a partial one; every channel gets the recorded channel's I/Q
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
@pytest.mark.parametrize("name", CHAIN_CASES)
def test_tap_is_the_sample_the_firmware_hands_its_modems(cuda, back, name, frames):
    import torch
    g, iq = rx_input(name)
    chain = U.RxChain(rx_config(g), channels=RX_C, frames=frames)
    tap = torch.zeros((RX_C, frames // 4), dtype=torch.float32, device="cuda")
    chain.set_digi_tap(tap)
    rows = []
    for k in range(iq.shape[1] // frames):
        chain.process(iq[:, k * frames:(k + 1) * frames].contiguous())
        chain.synchronize()
        rows.append(tap.clone())
    chain.close()
    check_tap(g, torch.cat(rows, dim=1).cpu().numpy())


@pytest.mark.parametrize("frames", [256, 2048])
def test_text_through_the_rx_chain(cuda, back, frames):
    """tap and text on leave audio and codec frames bit-identical; the text is the host decoder's on
    the chain's own tap and the reference's.  256-frame calls: against a chain with neither, the
    decoder reading the caller's tap row; 2048: the handle's own row, the tap from the other chain."""
    import torch
    name = CHAIN_CASES[0]
    g, iq = rx_input(name)
    cap = 256
    off_chain = U.RxChain(rx_config(g), channels=RX_C, frames=frames)
    on_chain = U.RxChain(rx_config(g), channels=RX_C, frames=frames)
    tap = torch.zeros((RX_C, frames // 4), dtype=torch.float32, device="cuda")
    (on_chain if frames == 256 else off_chain).set_digi_tap(tap)
    on_chain.set_rtty_text(True, *g["config"], text_capacity=cap)
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
            pieces = [a + b for a, b in zip(pieces, on_chain.rtty_text())]
    pieces = [a + b for a, b in zip(pieces, on_chain.rtty_text())]
    text, total = on_chain.rtty_text_outputs.read()
    rows = torch.cat(rows, dim=1).cpu().numpy()
    check_tap(g, rows)
    host = rtty.RttyDecoder(RX_C, *g["config"], capacity=cap, host=True)
    host.process(np.ascontiguousarray(rows))
    htext, htotal = host.read()
    assert np.array_equal(total, htotal) and np.array_equal(text, htext)
    check_text(g, text, total)
    assert pieces == [bytes(g["chars"])] * RX_C
    for ch in (off_chain, on_chain, host):
        ch.close()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_rx_pipelined_modes_give_the_serial_text(cuda, mode):
    """the decode launch follows the kernel that wrote the tap row on the side stream: calls enqueued
    back to back, no synchronisation between them (mode 3 runs as 2 with the tap on)"""
    g, iq = rx_input(CHAIN_CASES[0])
    frames = 256
    xs = [iq[:, k * frames:(k + 1) * frames].contiguous() for k in range(iq.shape[1] // frames)]
    out = []
    for m in (0, mode):
        chain = U.RxChain(rx_config(g), channels=RX_C, frames=frames)
        chain.set_pipelined(m)
        chain.set_rtty_text(True, *g["config"], text_capacity=256)
        for x in xs:
            chain.process(x)
        chain.join()
        chain.synchronize()
        out.append(chain.rtty_text_outputs.read())
        chain.close()
    check_text(g, *out[0])
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_rx_reset_restarts_the_decoder(cuda, back):
    g, iq = rx_input(CHAIN_CASES[1])
    frames = 2048
    chain = U.RxChain(rx_config(g), channels=RX_C, frames=frames)
    chain.set_rtty_text(True, *g["config"], text_capacity=256)
    runs = []
    for _ in range(2):
        for k in range(iq.shape[1] // frames):
            chain.process(iq[:, k * frames:(k + 1) * frames].contiguous())
        chain.synchronize()
        runs.append((chain.rtty_text_outputs.read(), chain.rtty_text()))
        chain.reset()
    check_text(g, *runs[0][0])
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a, b)
    assert runs[0][1] == runs[1][1]
    chain.close()


def test_rx_text_only_where_the_firmware_decodes(cuda):
    import torch
    refused = (dict(dmod_mode=U.DEMOD_USB, filter_path=48), dict(dmod_mode=U.DEMOD_SAM, filter_path=70),
               dict(dmod_mode=U.DEMOD_FM, filter_path=1), dict(dmod_mode=U.DEMOD_DIGI, filter_path=60))     # P60: 24 ksps
    for kw in refused:
        chain = U.RxChain(U.default_config(**kw), channels=4, frames=256)
        with pytest.raises(U.UhsdrError) as e:
            chain.set_rtty_text(True, *MAIN, text_capacity=64)
        assert e.value.status == U.UHSDR_ARGUMENT_ERROR and "rtty text" in str(e.value)
        # the tap itself: the 12 ksps SSB / CW / DIGI family only
        tap = torch.zeros((4, 64), dtype=torch.float32, device="cuda")
        if kw["dmod_mode"] == U.DEMOD_USB:
            chain.set_digi_tap(tap)
            chain.set_digi_tap(None)
        else:
            with pytest.raises(U.UhsdrError) as e:
                chain.set_digi_tap(tap)
            assert e.value.status == U.UHSDR_ARGUMENT_ERROR and "digi tap" in str(e.value)
        chain.close()
    chain = U.RxChain(U.default_config(dmod_mode=U.DEMOD_DIGI, filter_path=48), channels=4, frames=256)
    for bad in ((6, 0, 1, 0, 64), (1, 2, 1, 0, 64), (1, 0, 3, 0, 64), (1, 0, 1, 0, 4)):
        with pytest.raises(U.UhsdrError) as e:
            chain.set_rtty_text(True, *bad)
        assert e.value.status == U.UHSDR_ARGUMENT_ERROR
    with pytest.raises(RuntimeError):
        chain.rtty_text()
    with pytest.raises(ValueError):
        chain.set_digi_tap(torch.zeros((4, 63), dtype=torch.float32, device="cuda"))
    chain.set_rtty_text(True, *MAIN, text_capacity=8)
    chain.set_rtty_text(False)
    chain.close()
