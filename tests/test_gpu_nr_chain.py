"""The noise reduction and blanker inside the receive chain (uhsdr_rx_set_nr): rx_nr_head, the
12 ksps stream and rx_nr_tail against the reference firmware's whole chain with DSP NR, the blanker
or both on (tests/golden/nrchain_*.npz).  Everything is compared bit for bit over the whole
recording.

Shapes: head and tail run one wave per 64 channels with lane == channel and move their rows four
calls at a time, nr_frames four waves a block, nb_frames lane == channel -- so 1, 63, 65 and 130
channels, calls of 32 frames (one call a launch, a frame boundary inside a run of calls), 96 (a group
of three), 512 (four whole groups) and the whole recording (120 or 240 groups).  Each case holds two
recordings of one configuration, which alternate over the channels, so a lane that read its
neighbour's row or state would show.  Every output lies between guard words that must survive.

uhsdr_rx_nr_state is compared with the stand-alone host modules after the recorded nr_in: the three
noise-reduction words with uhsdr_nr_process_host's, the blanker's two counts with uhsdr_nb_*'s host
blanker on nr_in cut into the 128-sample frames the stream collects (the cases with the blanker are
not decimated, so the frames are nr_in's own)."""

import numpy as np
import pytest

import uhsdr_amd as U
from nr_chain_cases import CASES, load_case, nr_cfg, same_bits
from uhsdr_amd import nb, nr, rtty

pytestmark = pytest.mark.gpu

GUARD = 64                   # words of sentinel on both sides of every output
SENT_F, SENT_I = np.float32(-7.25e33), np.int32(-0x5A5A5A5B)
_dev = {}


def rx_config(g, **kw):
    return U.config_from_ref_args(dict(g["args"], **kw))


def tiled_iq(g, channels):
    """[channels][n][2] on the device, channel c holding recording c % 2"""
    import torch
    key = (g["name"], channels)
    if key not in _dev:
        _dev.clear()         # one case's input at a time on the device
        _dev[key] = torch.from_numpy(g["iq"][np.arange(channels) % 2]).cuda()
    return _dev[key]


class Guarded:
    """a contiguous device tensor of `shape` between two guards of sentinel words"""

    def __init__(self, shape, dtype):
        import torch
        self.sent = SENT_F if dtype == torch.float32 else SENT_I
        self.n = int(np.prod(shape))
        self.flat = torch.full((self.n + 2 * GUARD,), float(self.sent) if dtype == torch.float32 else int(self.sent), dtype=dtype, device="cuda")
        self.t = self.flat[GUARD:GUARD + self.n].view(*shape)

    def intact(self):
        f = self.flat.cpu().numpy()
        return bool((f[:GUARD] == self.sent).all() and (f[GUARD + self.n:] == self.sent).all())


def run(g, channels, frames, calls=None, nr_kw=None, tap=False, text=False, mchf=False):
    """the case through a chain with the stage on; returns the chain and the outputs as arrays"""
    import torch
    iq = tiled_iq(g, channels)
    chain = U.RxChain(rx_config(g), channels=channels, frames=frames)
    chain.set_nr(nr_cfg(g, **(nr_kw or {})))
    audio, dst = Guarded((channels, frames), torch.float32), Guarded((channels, frames, 2), torch.int32)
    a0 = Guarded((channels, frames), torch.float32) if mchf else None
    tp = Guarded((channels, frames // 4), torch.float32) if tap else None
    if tap:
        chain.set_digi_tap(tp.t)
    if text:
        chain.set_rtty_text(True, 1, 0, 1, 0, text_capacity=64)
    out = dict(audio=[], dst=[], a0=[], tap=[])
    n = iq.shape[1] // frames if calls is None else calls
    for k in range(n):
        x = iq[:, k * frames:(k + 1) * frames].contiguous()
        if mchf:
            chain.process_stereo(x, audio.t, a0.t, dst.t)
        else:
            chain.process(x, audio.t, dst.t)
        out["audio"].append(audio.t.clone()); out["dst"].append(dst.t.clone())
        if mchf:
            out["a0"].append(a0.t.clone())
        if tap:
            out["tap"].append(tp.t.clone())
    chain.synchronize()
    for b in (audio, dst, a0, tp):
        assert b is None or b.intact(), "a guard word was overwritten"
    return chain, {k: torch.cat(v, dim=1).cpu().numpy() for k, v in out.items() if v}


def check(g, got, key, ref_key=None):
    ref = g[ref_key or key]
    n = got[key].shape[1]
    for c in range(got[key].shape[0]):
        r = ref[c % 2][:n]
        if not same_bits(got[key][c], r):
            bad = np.flatnonzero((np.ascontiguousarray(got[key][c]).view(np.uint32) != np.ascontiguousarray(r).view(np.uint32)).reshape(n, -1).any(axis=1))
            raise AssertionError(f"{g['name']} {key} channel {c}: {len(bad)} of {n} differ, first at {bad[0]}")


def host_state(g):
    p = nr.NrProcessor(2, nr_cfg(g), host=True)
    x = np.ascontiguousarray(g["nr_in"])
    p.process(x, np.empty_like(x))
    s = p.state()
    p.close()
    return s


def host_blanker_state(g):
    """(last, total) of the stand-alone host blanker after the whole frames of the recorded nr_in"""
    assert g["nr"]["width_hz"] >= 2701                      # not decimated: the stream's frames are nr_in's
    p = nb.NbProcessor(2, nb.nb_config(nb_setting=g["nr"]["nb_setting"]), host=True)
    x = np.array(g["nr_in"][:, :g["nr_in"].shape[1] // nb.FRAME * nb.FRAME])
    p.process_frames(x)
    s = p.state()
    p.close()
    return s


def check_state(g, chain, channels):
    ft, nn, pr, last, tot = chain.nr_state()
    want = host_state(g)
    idx = np.arange(channels) % 2
    if not g["nr"]["nr_bypass"]:
        assert np.array_equal(ft, want[0][idx]) and np.array_equal(nn, want[1][idx]) and same_bits(pr, want[2][idx])
    if g["nr"]["nb_setting"] == 0:
        assert not tot.any() and not last.any()
    else:
        hlast, htot = host_blanker_state(g)
        assert (htot > 0).all() and (htot != hlast).all()   # the recordings with clicks; a swap of the two would show
        assert last.dtype == hlast.dtype and tot.dtype == htot.dtype
        assert np.array_equal(last, hlast[idx]) and np.array_equal(tot, htot[idx])


SHAPES = [(name, 65, 512) for name in CASES] + [
    ("ssb_wide", 1, 32), ("ssb_wide", 63, 15360), ("ssb_wide", 130, 512), ("ssb_narrow", 63, 96), ("ssb_narrow", 1, 30720),
    ("nb_nr", 63, 32), ("nb_nr", 1, 15360), ("nb", 1, 96), ("nb", 63, 15360), ("cw", 63, 32), ("notch", 1, 96), ("mchf", 63, 32),
    ("mchf", 1, 15360), ("digi", 63, 96),
]


@pytest.mark.parametrize("name,channels,frames", SHAPES)
def test_audio_is_the_firmwares_with_the_stage_on(cuda, name, channels, frames):
    g = load_case(name)
    mchf = "dst" in g
    chain, got = run(g, channels, frames, mchf=mchf)
    check(g, got, "audio")
    if mchf:
        check(g, got, "dst")
        check(g, got, "a0")
    else:
        # OVI40: both codec words are the audio converted (audio_driver.c:2911-2923)
        assert np.array_equal(got["dst"][..., 0], got["dst"][..., 1])
    check_state(g, chain, channels)
    chain.close()


@pytest.mark.parametrize("channels,frames,text", [(65, 512, True), (1, 32, False), (63, 15360, True)])
def test_tap_and_text_see_the_noise_reduced_sample(cuda, channels, frames, text):
    g = load_case("digi")
    chain, got = run(g, channels, frames, tap=True, text=text)
    check(g, got, "audio")
    check(g, got, "tap")
    if text:
        dtext, dtotal = chain.rtty_text_outputs.read()
        host = rtty.RttyDecoder(2, 1, 0, 1, 0, capacity=64, host=True)
        host.process(np.ascontiguousarray(g["tap"]))
        htext, htotal = host.read()
        idx = np.arange(channels) % 2
        assert np.array_equal(dtotal, htotal[idx]) and np.array_equal(dtext, htext[idx])
        host.close()
    chain.close()


@pytest.mark.parametrize("name,channels,frames", [("ssb_narrow", 65, 512), ("cw", 63, 96)])
def test_tap_on_the_paths_without_an_anti_alias_lattice(cuda, name, channels, frames):
    """the tail instance with the tap of the narrow paths (interpolator phase 4, no lattice behind it):
    the audio stays the firmware's, and the tap row, for which these cases hold no recording, is one
    row per recording, finite and not silent, with its guards intact"""
    g = load_case(name)
    chain, got = run(g, channels, frames, tap=True)
    assert U.build_plan(rx_config(g)).aa_stages == 0
    check(g, got, "audio")
    tap = got["tap"]
    assert np.isfinite(tap).all() and np.abs(tap[:, tap.shape[1] // 2:]).max() > 1.0
    for c in range(2, channels):
        assert same_bits(tap[c], tap[c - 2]), c
    if channels > 1:
        assert not same_bits(tap[0], tap[1])
    chain.close()


def test_tap_row_alignment_with_the_stage_on(cuda):
    """the tail stores the tap row in 16-byte pieces: a row that is not aligned so is refused by
    whichever of set_digi_tap and set_nr comes second, and is fine with the stage off"""
    import torch
    g = load_case("digi")
    frames = 512
    chain = U.RxChain(rx_config(g), channels=4, frames=frames)
    flat = torch.zeros(4 * frames // 4 + 8, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    odd, even = flat[1:1 + 4 * frames // 4].view(4, frames // 4), flat[4:4 + 4 * frames // 4].view(4, frames // 4)
    chain.set_digi_tap(odd)
    refused(chain.set_nr, nr_cfg(g))
    refused(chain.nr_state)                                 # the stage stayed off
    chain.set_digi_tap(even)
    chain.set_nr(nr_cfg(g))
    refused(chain.set_digi_tap, odd)
    chain.set_nr(None)
    chain.set_digi_tap(odd)
    chain.close()


def test_cw_front_end_and_text_behind_the_stage(cuda):
    """the CW decoder's signal row and the Morse text run on the tail's samples: the audio stays the
    firmware's with them on, and every channel of one recording decodes the same"""
    import torch
    g = load_case("cw")
    channels, frames = 65, 512
    iq = tiled_iq(g, channels)
    chain = U.RxChain(rx_config(g), channels=channels, frames=frames)
    chain.set_nr(nr_cfg(g))
    chain.set_cw_text(True, 0, 64)
    sig = torch.zeros((channels, frames // 32), dtype=torch.uint8, device="cuda")
    chain.set_cw_outputs(sig, None)
    audio = torch.empty((channels, frames), dtype=torch.float32, device="cuda")
    rows, sigs = [], []
    for k in range(iq.shape[1] // frames):
        chain.process(iq[:, k * frames:(k + 1) * frames].contiguous(), audio)
        rows.append(audio.clone()); sigs.append(sig.clone())
    chain.synchronize()
    check(g, dict(audio=torch.cat(rows, dim=1).cpu().numpy()), "audio")
    s = torch.cat(sigs, dim=1).cpu().numpy()
    assert s.any() and not s.all()
    assert np.array_equal(s[2:], s[:-2])
    text = chain.cw_text()
    assert text[2:] == text[:-2]
    chain.close()


def test_reset_and_a_new_stage_start_fresh(cuda):
    g = load_case("nb_nr")
    channels, frames, calls = 65, 512, 8
    chain, first = run(g, channels, frames, calls=calls)
    check(g, first, "audio")
    import torch
    iq = tiled_iq(g, channels)
    audio = torch.empty((channels, frames), dtype=torch.float32, device="cuda")

    def again():
        rows = []
        for k in range(calls):
            chain.process(iq[:, k * frames:(k + 1) * frames].contiguous(), audio)
            rows.append(audio.clone())
        return dict(audio=torch.cat(rows, dim=1).cpu().numpy())
    chain.reset()
    check(g, again(), "audio")
    # a new configuration is a fresh stage too; the chain's own state needs the reset
    chain.set_nr(nr_cfg(g))
    chain.reset()
    check(g, again(), "audio")
    chain.close()


def test_off_again_reads_no_stale_rows(cuda):
    """Two handles through the same calls with the stage on, then off: what follows is equal bit for
    bit and finite, so no freed or unwritten row is read.  The pre-filter, the AGC and the front never
    saw the stage: after a reset such a handle gives what a handle gives whose stage was never on."""
    import torch
    g = load_case("ssb_wide")
    channels, frames = 65, 512
    iq = tiled_iq(g, channels)
    chains = [U.RxChain(rx_config(g), channels=channels, frames=frames) for _ in range(2)]
    audio = [torch.empty((channels, frames), dtype=torch.float32, device="cuda") for _ in range(2)]
    for ch in chains:
        ch.set_nr(nr_cfg(g))
    for k in range(10):
        x = iq[:, k * frames:(k + 1) * frames].contiguous()
        for ch, a in zip(chains, audio):
            ch.process(x, a)
    for ch in chains:
        ch.set_nr(None)
        with pytest.raises(U.UhsdrError):
            ch.nr_state()
    for k in range(10, 20):
        x = iq[:, k * frames:(k + 1) * frames].contiguous()
        for ch, a in zip(chains, audio):
            ch.process(x, a)
        torch.cuda.synchronize()
        assert torch.equal(audio[0].view(torch.int32), audio[1].view(torch.int32)), k
        assert np.isfinite(audio[0].cpu().numpy()).all()
    # the pre-filter and the AGC never saw the stage: after a reset the handle is the one it always was
    fresh = U.RxChain(rx_config(g), channels=channels, frames=frames)
    chains[0].reset()
    for k in range(4):
        x = iq[:, k * frames:(k + 1) * frames].contiguous()
        chains[0].process(x, audio[0])
        fresh.process(x, audio[1])
        torch.cuda.synchronize()
        assert torch.equal(audio[0].view(torch.int32), audio[1].view(torch.int32)), k
    for ch in chains + [fresh]:
        ch.close()


def refused(fn, *a):
    with pytest.raises(U.UhsdrError) as e:
        fn(*a)
    assert e.value.status == U.UHSDR_ARGUMENT_ERROR, str(e.value)


def test_refusals(cuda):
    import torch
    cfg = nr.nr_config(width_hz=3800, offset_hz=1900)
    frames = 512
    # every other path family
    for kw in (dict(filter_path=55), dict(dmod_mode=U.DEMOD_AM, filter_path=70), dict(dmod_mode=U.DEMOD_SAM, filter_path=70),
               dict(dmod_mode=U.DEMOD_FM, filter_path=1), dict(dmod_mode=U.DEMOD_SSBSTEREO, filter_path=48, stereo_enable=1)):
        chain = U.RxChain(U.default_config(**kw), channels=4, frames=frames)
        refused(chain.set_nr, cfg)
        chain.set_nr(None)                                   # off stays off
        chain.close()
    g = load_case("ssb_wide")
    chain = U.RxChain(rx_config(g), channels=4, frames=frames)
    iq = tiled_iq(g, 4)
    audio = torch.empty((4, frames), dtype=torch.float32, device="cuda")
    # what uhsdr_nr_create refuses, before anything changes
    for bad in (dict(nr_bypass=1), dict(nb_setting=16), dict(asnr=1), dict(width=6), dict(alpha=1.5), dict(width_hz=200, offset_hz=2990)):
        refused(chain.set_nr, nr_cfg(g, **bad))
        refused(chain.nr_state)
    # the modes it is not built in
    for m in (1, 2, 3):
        chain.set_pipelined(m)
        refused(chain.set_nr, cfg)
    chain.set_pipelined(0)
    chain.set_schedule(U.SCHEDULE_CHAIN)
    refused(chain.set_nr, cfg)
    chain.set_schedule(U.SCHEDULE_SPLIT_FUSED)
    chain.set_precision(U.PRECISION_FMA)
    refused(chain.set_nr, cfg)
    chain.set_precision(U.PRECISION_EXACT)
    # sample_rate is the stream's own decision
    chain.set_nr(nr_cfg(g, sample_rate=1))
    # and with it on, the way into them
    chain.set_nr(nr_cfg(g))
    for m in (1, 2, 3):
        refused(chain.set_pipelined, m)
    refused(chain.set_schedule, U.SCHEDULE_CHAIN)
    refused(chain.set_precision, U.PRECISION_FMA)
    chain.set_pipelined(0)
    chain.set_schedule(U.SCHEDULE_SPLIT_PIPE)
    # a refused configuration leaves the running stage alone: the audio stays the firmware's
    rows = []
    for k in range(iq.shape[1] // frames):
        if k == 7:
            refused(chain.set_nr, nr_cfg(g, asnr=31))
        chain.process(iq[:, k * frames:(k + 1) * frames].contiguous(), audio)
        rows.append(audio.clone())
    check(g, dict(audio=torch.cat(rows, dim=1).cpu().numpy()), "audio")
    chain.close()


def test_set_stream_moves_the_stage(cuda):
    import torch
    g = load_case("ssb_wide")
    channels, frames = 63, 512
    iq = tiled_iq(g, channels)
    chain = U.RxChain(rx_config(g), channels=channels, frames=frames)
    chain.set_nr(nr_cfg(g))
    audio = torch.empty((channels, frames), dtype=torch.float32, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    rows = []
    for k in range(iq.shape[1] // frames):
        x = iq[:, k * frames:(k + 1) * frames].contiguous()
        if k % 5 == 2:
            torch.cuda.synchronize()                        # x and the clones above are on torch's stream
            chain.set_stream(streams[(k // 5) % 2].cuda_stream)
        chain.process(x, audio)
        chain.synchronize()
        rows.append(audio.clone())
    check(g, dict(audio=torch.cat(rows, dim=1).cpu().numpy()), "audio")
    chain.close()
