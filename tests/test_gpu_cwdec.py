"""CW decoder back end on the device (cw_decode, uhsdr_cwdec.hip): the stand-alone decoder against
the reference firmware's recorded output (tests/golden/cwtext_*.npz) with a different case on each
lane, against the host build of the same step function on arbitrary input, and inside the RX
chain.  Everything is compared exactly."""
import numpy as np
import pytest

import uhsdr_amd as U
from test_cwdec_host import CASES, load_case
from uhsdr_amd import cwdec, synth

pytestmark = pytest.mark.gpu


def group(blocksize, spikecancel):
    return [g for g in (load_case(n) for n in CASES) if int(g["blocksize"]) == blocksize and int(g["spikecancel"]) == spikecancel]


class Tiled:
    """cases of one (blocksize, spikecancel) over C channels, channel c running case c % n; rows
    padded with space to the longest case, every channel checked up to its own case's length"""

    def __init__(self, cases, C, shift=0):
        self.g = [cases[(c + shift) % len(cases)] for c in range(C)]
        self.len = np.array([len(g["state"]) for g in self.g])
        self.blocks = int(self.len.max())
        self.state = np.zeros((C, self.blocks), np.uint8)
        for c, g in enumerate(self.g):
            self.state[c, :self.len[c]] = g["state"]

    def expect(self, bounds):
        """per channel and bound: characters emitted so far, the WPM byte, and whether the case reaches that far"""
        bounds = np.asarray(bounds)
        self.want_total = np.stack([np.searchsorted(g["char_block"], bounds, "left") for g in self.g])
        self.want_wpm = np.stack([g["speed"][np.minimum(bounds, len(g["speed"])) - 1] for g in self.g])
        self.valid = bounds[None, :] <= self.len[:, None]

    def check(self, i, done, text, total, wpm, cap, ring=True):
        v = self.valid[:, i]
        assert np.array_equal(total[v], self.want_total[v, i]), done
        assert np.array_equal(wpm[v], self.want_wpm[v, i]), done
        if ring:
            for c in np.flatnonzero(v):
                n = int(total[c])
                k = np.arange(max(0, n - cap), n)
                assert bytes(text[c, k % cap]) == bytes(self.g[c]["chars"][k]), (c, done)


def feed(t, dec, bounds, cap, ring_every=1):
    import torch
    state = torch.from_numpy(t.state).cuda()
    t.expect(bounds)
    last = 0
    for i, b in enumerate(bounds):
        dec.process(state[:, last:b].contiguous())
        text, total, wpm = dec.read()
        t.check(i, b, text, total, wpm, cap, ring=(i % ring_every == 0 or b == bounds[-1]))
        last = b


@pytest.mark.parametrize("C,per_call,cap", [(1, None, 64), (63, None, 8), (65, None, 64), (130, None, 8),
                                            (1, 5, 8), (63, 5, 64), (65, 5, 8), (130, 5, 64),
                                            (1, 64, 64), (63, 64, 8), (65, 64, 64), (130, 64, 8)])
def test_fixtures_tiled_over_lanes(cuda, C, per_call, cap):
    t = Tiled(group(88, 0), C, shift=C)
    dec = cwdec.CwDecoder(C, 88, 0, cap)
    if per_call is None:
        bounds = sorted(set(int(x) for x in t.len))      # one piece, up to each case's end
    else:
        bounds = list(range(per_call, t.blocks, per_call)) + [t.blocks]
    feed(t, dec, bounds, cap, ring_every=16)
    dec.close()


@pytest.mark.parametrize("blocksize,spikecancel", [(60, 0), (128, 0), (60, 1), (88, 2)])
def test_other_block_sizes_and_spike_modes(cuda, blocksize, spikecancel):
    t = Tiled(group(blocksize, spikecancel), 65)
    dec = cwdec.CwDecoder(65, blocksize, spikecancel, 8)
    feed(t, dec, sorted(set(int(x) for x in t.len)), 8)
    dec.close()


def test_one_block_per_call(cuda):
    import torch
    t = Tiled(group(88, 0), 65)
    dec = cwdec.CwDecoder(65, 88, 0, 64)
    state = torch.from_numpy(t.state[:, :4096]).cuda()
    cols = [state[:, b:b + 1].contiguous() for b in range(4096)]
    bounds = list(range(8, 4097, 8))
    t.expect(bounds)
    for b in range(4096):
        dec.process(cols[b])
        if b % 8 == 7:
            text, total, wpm = dec.read()
            t.check(b // 8, b + 1, text, total, wpm, 64, ring=(b % 256 == 255))
    dec.close()


def random_states(C, blocks, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for c in range(C):
        runs = rng.integers(1, 3 + 5 * (c % 7), size=blocks)
        rows.append(np.repeat((np.arange(len(runs)) + c) % 2, runs)[:blocks].astype(np.uint8))
    return np.ascontiguousarray(np.stack(rows))


@pytest.mark.parametrize("per_call", [2048, 100])
def test_device_equals_host_on_arbitrary_input(cuda, per_call):
    import torch
    state = random_states(130, 2048, 20261020)
    host = cwdec.CwDecoder(130, 72, 2, 64, host=True)
    host.process(state)
    want = host.read()
    assert int(want[1].sum()) > 130 and (want[0] == ord("#")).any()      # text, error paths included
    dec = cwdec.CwDecoder(130, 72, 2, 64)
    d = torch.from_numpy(state).cuda()
    for b in range(0, 2048, per_call):
        dec.process(d[:, b:b + per_call].contiguous())
    for got, ref in zip(dec.read(), want):
        assert np.array_equal(got, ref)
    dec.reset()
    dec.process(d)
    for got, ref in zip(dec.read(), want):
        assert np.array_equal(got, ref)
    dec.close()
    host.close()


# ---- through the RX chain ----

MSG = "CQ DE UHSDR K"
RX_C, RX_N, SIDETONE = 65, 844 * 2048, 500     # 36 s; path 4's 300 Hz filter passes 500 Hz
_rx = {}


def rx_config(thresh):
    return U.default_config(dmod_mode=U.DEMOD_CW, filter_path=4, cw_decoder_blocksize=88, cw_sidetone_freq=SIDETONE,
                            cw_decoder_thresh=int(thresh))


def rx_input():
    """the keyed I/Q on the device, and a threshold from the chain's own Goertzel energies: a fifth
    of the largest energy of the first 3.5 s"""
    import torch
    if not _rx:
        iq = torch.empty((RX_C, RX_N, 2), dtype=torch.int32, device="cuda")
        step = 32 * 2048
        for off in range(0, RX_N, step):
            n = min(step, RX_N - off)
            iq[:, off:off + n] = torch.from_numpy(synth.cw_text_iq(np.arange(RX_C), off, n, MSG, 20.0, noise_sigma=0.0,
                                                                   tone=float(SIDETONE)))
        chain = U.RxChain(rx_config(1000), channels=RX_C, frames=2048)
        en = torch.zeros((RX_C, chain.cw_blocks_max), dtype=torch.float32, device="cuda")
        chain.set_cw_outputs(None, en)
        peak = 0.0
        for k in range(82):
            chain.process(iq[:, k * 2048:(k + 1) * 2048].contiguous())
            chain.synchronize()
            peak = max(peak, float(en[:, :chain.cw_blocks_last].max()))
        chain.close()
        _rx["iq"], _rx["thresh"] = iq, 0.2 * peak
    return _rx["iq"], _rx["thresh"]


def block_calls(total_calls, blocksize=88, ndc=8):
    """the 32-frame calls at which CwDecode_RxProcessor completes a block"""
    out, count = [], 0
    for j in range(total_calls):
        count += ndc
        if count >= blocksize:
            out.append(j)
            count = 0
    return np.array(out)


@pytest.mark.parametrize("frames", [256, 2048])
def test_text_through_the_rx_chain(cuda, back, frames):
    import torch
    iq, thresh = rx_input()
    cfg = rx_config(thresh)
    off_chain = U.RxChain(cfg, channels=RX_C, frames=frames)
    on_chain = U.RxChain(cfg, channels=RX_C, frames=frames)
    sig = [torch.zeros((RX_C, frames // 32), dtype=torch.uint8, device="cuda") for _ in range(2)]
    en = [torch.zeros((RX_C, off_chain.cw_blocks_max), dtype=torch.float32, device="cuda") for _ in range(2)]
    audio = [torch.empty((RX_C, frames), dtype=torch.float32, device="cuda") for _ in range(2)]
    off_chain.set_cw_outputs(sig[0], en[0])
    # the decoder reads the caller's signal row (256-frame calls) or the handle's own (2048)
    on_chain.set_cw_outputs(sig[1] if frames == 256 else None, en[1])
    on_chain.set_cw_text(True, 0, 4096)
    rows, pieces = [], [b""] * RX_C
    for k in range(RX_N // frames):
        x = iq[:, k * frames:(k + 1) * frames].contiguous()
        off_chain.process(x, audio[0], None)
        on_chain.process(x, audio[1], None)
        torch.cuda.synchronize()
        nb = off_chain.cw_blocks_last
        assert on_chain.cw_blocks_last == nb
        # text on leaves the chain's outputs bit-identical
        assert torch.equal(audio[0].view(torch.int32), audio[1].view(torch.int32)), k
        assert torch.equal(en[0][:, :nb].view(torch.int32), en[1][:, :nb].view(torch.int32)), k
        if frames == 256:
            assert torch.equal(sig[0], sig[1]), k
        rows.append(sig[0].clone())
        if k % 97 == 0:
            pieces = [a + b for a, b in zip(pieces, on_chain.cw_text())]
    pieces = [a + b for a, b in zip(pieces, on_chain.cw_text())]
    signal = torch.cat(rows, dim=1).cpu().numpy()
    text, total, wpm = on_chain.cw_text_outputs.read()

    # the host decoder on the chain's own signal row at the block-completion calls
    states = np.ascontiguousarray(signal[:, block_calls(RX_N // 32)])
    host = cwdec.CwDecoder(RX_C, 88, 0, 4096, host=True)
    host.process(states)
    htext, htotal, hwpm = host.read()
    assert np.array_equal(total, htotal) and np.array_equal(wpm, hwpm) and np.array_equal(text, htext)
    want = " ".join([MSG] * 3).encode()
    for c in range(RX_C):
        got = bytes(text[c, :int(total[c])])
        assert pieces[c] == got, c
        assert want in got[len(MSG):], (c, got)      # past the garbled start: the third to fifth repetitions, verbatim
    off_chain.close()
    on_chain.close()
    host.close()


def test_rx_reset_restarts_the_decoder(cuda, back):
    iq, thresh = rx_input()
    chain = U.RxChain(rx_config(thresh), channels=RX_C, frames=2048)
    chain.set_cw_text(True, 0, 64)
    runs = []
    for _ in range(2):
        for k in range(16 * 48000 // 2048):      # text starts once 98 states have set the timing, about 10 s in
            chain.process(iq[:, k * 2048:(k + 1) * 2048].contiguous())
        chain.synchronize()
        runs.append((chain.cw_text_outputs.read(), chain.cw_text()))
        chain.reset()
    assert int(runs[0][0][1].min()) > 8
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a, b)
    assert runs[0][1] == runs[1][1]
    chain.close()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_rx_pipelined_modes_give_the_serial_text(cuda, mode):
    """the decode launch follows the kernel that wrote the signal row on the side stream: calls
    enqueued back to back, no synchronisation between them (mode 3 runs as 2 with the CW front end)"""
    iq, thresh = rx_input()
    frames, calls = 256, 16 * 48000 // 256
    xs = [iq[:, k * frames:(k + 1) * frames].contiguous() for k in range(calls)]
    out = []
    for m in (0, mode):
        chain = U.RxChain(rx_config(thresh), channels=RX_C, frames=frames)
        chain.set_pipelined(m)
        chain.set_cw_text(True, 0, 64)
        for x in xs:
            chain.process(x)
        chain.join()
        chain.synchronize()
        out.append(chain.cw_text_outputs.read())
        chain.close()
    assert int(out[0][1].min()) > 8
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_rx_text_only_where_the_firmware_decodes(cuda):
    for kw in (dict(dmod_mode=U.DEMOD_USB, filter_path=48), dict(dmod_mode=U.DEMOD_SAM, filter_path=70)):
        chain = U.RxChain(U.default_config(**kw), channels=4, frames=256)
        with pytest.raises(U.UhsdrError) as e:
            chain.set_cw_text(True, 0, 64)
        assert e.value.status == U.UHSDR_ARGUMENT_ERROR and "cw text" in str(e.value)
        chain.close()
    chain = U.RxChain(rx_config(1000), channels=4, frames=256)
    for bad in ((3, 64), (0, 4)):
        with pytest.raises(U.UhsdrError) as e:
            chain.set_cw_text(True, *bad)
        assert e.value.status == U.UHSDR_ARGUMENT_ERROR
    with pytest.raises(RuntimeError):
        chain.cw_text()
    chain.set_cw_text(True, 2, 8)
    chain.set_cw_text(False)
    chain.close()
