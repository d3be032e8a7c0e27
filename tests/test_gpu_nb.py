"""Noise blanker on the device (nb_frames, uhsdr_nb.hip, and the stream of uhsdr_nr.hip with the
blanker in it) against the reference firmware's recorded output (tests/golden/nb_*.npz) with a
different case on each channel, and against the host build of the same step functions on arbitrary
seeded input.  Everything is compared exactly (a NaN equals a NaN).  nb_frames runs a channel per
lane, one wave per block: 1, 3, 63, 65 and 130 channels give a partial wave, a wave less one, a wave
plus one and two waves plus a part."""
import ctypes as C

import numpy as np
import pytest

import uhsdr_amd as U
import nr_cases
from nb_cases import FRAME, SHOW, STREAM_SHOW, check_frames, load_case, load_stream_case, same, stream_config_of
from uhsdr_amd import nb, nr

pytestmark = pytest.mark.gpu

SETTING_8 = sorted(n for n, (s, _) in SHOW.items() if s == 8)       # one setting, ten inputs
PAD = 24


def device_frames(cuda, cfg, rows, frames, sizes, in_place=False):
    """rows [C][frames * 128] through a device blanker in calls of `sizes` frames (cycled; None: one
    call), on rows PAD floats longer than the run and filled with 7.0 behind it; the output and the state"""
    import torch
    channels, n = rows.shape[0], frames * FRAME
    x = np.full((channels, n + PAD), 7.0, np.float32)
    x[:, :n] = rows[:, :n]
    dx = torch.from_numpy(x).to(cuda)
    dy = dx if in_place else torch.full_like(dx, 7.0)
    p = nb.NbProcessor(channels, cfg)
    at, i = 0, 0
    while at < frames:
        k = frames - at if sizes is None else min(sizes[i % len(sizes)], frames - at)
        U._abi.check(p.lib.uhsdr_nb_process_frames(p.handle, C.c_void_p(dx.data_ptr() + 4 * at * FRAME),
                                                   C.c_void_p(dy.data_ptr() + 4 * at * FRAME), k, n + PAD), "uhsdr_nb_process_frames")
        at += k
        i += 1
    state = p.state()
    y = dy.cpu().numpy()
    assert (y[:, n:] == 7.0).all()                          # nothing is written past the run
    p.close()
    return y[:, :n], state


def host_frames(cfg, rows, frames):
    x = np.ascontiguousarray(rows[:, :frames * FRAME])
    y = np.zeros_like(x)
    p = nb.NbProcessor(x.shape[0], cfg, host=True)
    p.process_frames(x, y)
    return y, p.state()


@pytest.mark.parametrize("channels,sizes,in_place", [(1, [1], False), (3, [19], True), (63, None, False), (65, [19], False), (130, None, True),
                                                     (65, [1], False)])
def test_fixtures_one_case_per_channel(cuda, channels, sizes, in_place):
    gs = [load_case(n) for n in SETTING_8]
    mine = [gs[(c + channels) % len(gs)] for c in range(channels)]
    frames = gs[0]["frames"]
    rows = np.stack([g["audio"] for g in mine])
    y, (last, total) = device_frames(cuda, nb.nb_config(nb_setting=8), rows, frames, sizes, in_place)
    for c, g in enumerate(mine):
        check_frames(g, y[c], what=f"channel {c}")
    hy, (hlast, htotal) = host_frames(nb.nb_config(nb_setting=8), rows, frames)
    assert same(y, hy).all() and np.array_equal(last, hlast) and np.array_equal(total, htotal)
    for c, g in enumerate(mine):
        assert (total[c] > 0) == bool(g["changed"].any()), (c, g["name"])


@pytest.mark.parametrize("name", sorted(n for n, (s, _) in SHOW.items() if s != 8))
def test_other_settings(cuda, name):
    """the recordings at settings 1 and 15: the case, its mirror image and a copy 40 dB down"""
    g = load_case(name)
    x = g["audio"]
    rows = np.stack([x, -x, x * np.float32(0.01)])
    cfg = nb.nb_config(**g["cfg"])
    y, state = device_frames(cuda, cfg, rows, g["frames"], [7, 19, 1])
    check_frames(g, y[0])
    assert np.array_equal(y[1], -y[0])                      # the blanker is odd in its input
    hy, hstate = host_frames(cfg, rows, g["frames"])
    assert same(y, hy).all() and np.array_equal(state[0], hstate[0]) and np.array_equal(state[1], hstate[1])


def arbitrary_rows(channels, frames):
    """seeded noise at amplitudes from 1e-20 to 1e15 with impulses on half the channels, a silent
    channel, one that falls silent, one with a NaN and one with an infinity in it"""
    rng = np.random.default_rng(43)
    n = frames * FRAME
    rows = rng.standard_normal((channels, n))
    for c in range(0, channels, 2):                         # coloured, so that the predictor has something to predict
        rows[c] = np.convolve(rows[c], [1.0, 1.6, 1.2, 0.5], mode="same")
    for c in range(channels // 2):
        at = rng.integers(0, n, 12)
        rows[c, at] += rng.choice([-1.0, 1.0], 12) * rng.uniform(5.0, 60.0, 12)
    rows = (rows * 10.0 ** rng.uniform(-20, 15, (channels, 1))).astype(np.float32)
    rows[10] = 0.0
    rows[11, 9 * FRAME + 40:] = 0.0
    rows[12, 7 * FRAME + 5] = np.nan
    rows[13, 5 * FRAME + 120] = np.inf
    return rows


def test_arbitrary_input_against_the_host_twin(cuda):
    """65 channels at every setting 1 .. 15 in turn, through separate handles"""
    channels, frames = 65, 20
    rows = arbitrary_rows(channels, frames)
    busy = set()
    for setting in range(1, 16):
        cfg = nb.nb_config(nb_setting=setting)
        y, (last, total) = device_frames(cuda, cfg, rows, frames, [3, 16, 1], in_place=setting % 2 == 0)
        hy, (hlast, htotal) = host_frames(cfg, rows, frames)
        bad = np.argwhere(~same(y, hy))
        assert len(bad) == 0, (setting, "first difference at channel, sample", bad[0].tolist(), "of", len(bad))
        assert np.array_equal(last, hlast) and np.array_equal(total, htotal), setting
        assert total[10] == 0 and last.max() <= nb.MAX_HITS
        busy.add(int((total > 0).sum()))
    assert max(busy) > channels // 2 and len(busy) > 3      # the settings differ in what they repair


def device_stream(cuda, cfg, rows, calls):
    import torch
    channels, n = rows.shape
    dx = torch.from_numpy(np.ascontiguousarray(rows)).to(cuda)
    dy = torch.zeros_like(dx)
    p = nr.NrProcessor(channels, cfg)
    at = 0
    for k in calls:
        U._abi.check(p.lib.uhsdr_nr_process(p.handle, C.c_void_p(dx.data_ptr() + 4 * at), C.c_void_p(dy.data_ptr() + 4 * at), k, n),
                     "uhsdr_nr_process")
        at += k
    assert at == n
    y = dy.cpu().numpy()
    p.close()
    return y


def host_stream(cfg, rows):
    y = np.zeros_like(rows)
    p = nr.NrProcessor(rows.shape[0], cfg, host=True)
    p.process(np.ascontiguousarray(rows), y)
    return y


@pytest.mark.parametrize("name", sorted(STREAM_SHOW))
@pytest.mark.parametrize("calls", ["8", "large"])
def test_stream(cuda, name, calls):
    """65 channels: channel 0 the recorded case, the others scaled copies; 600 calls of 8 samples, or
    one large call and the remainder"""
    g = load_stream_case(name)
    gains = (10.0 ** np.linspace(0.0, -3.0, 65)).astype(np.float32)
    rows = g["audio"][None, :] * gains[:, None]
    cfg = stream_config_of(g)
    y = device_stream(cuda, cfg, rows, [8] * 600 if calls == "8" else [4000, 8, 792])
    bad = np.flatnonzero(~same(y[0], g["out"]))
    assert len(bad) == 0, (name, calls, "first differing sample", int(bad[0]), "of", len(bad))
    assert same(y, host_stream(cfg, rows)).all()


def test_stream_without_the_blanker_is_unchanged(cuda):
    """both new fields 0: the existing stream recording through a device handle"""
    g = nr_cases.load_stream_case("ssb")
    cfg = nr_cases.config_of(g)
    assert cfg.nb_setting == 0 and cfg.nr_bypass == 0
    x = g["audio"]
    y = device_stream(cuda, cfg, np.stack([x, -x, x[::-1]]), [4000, 8, 3000, 992])
    assert np.array_equal(y[0].view(np.uint32), g["out"].view(np.uint32))


def test_frames_through_the_noise_reduction_handle_and_reset(cuda):
    import torch
    g = load_case("walk")
    x = np.array(g["audio"][None, :])
    dx = torch.from_numpy(x).to(cuda)
    dy = torch.zeros_like(dx)
    p = nr.NrProcessor(1, nr.nr_config(nb_setting=8, nr_bypass=1, sample_rate=12000, width_hz=3200, offset_hz=1700))
    p.process_frames(dx, dy, frames=30)
    p.reset()
    p.process_frames(dx, dy)
    check_frames(g, dy.cpu().numpy()[0])
    p.close()
    cfg = nr.nr_config(nb_setting=8, sample_rate=12000, width_hz=3200, offset_hz=1700)
    q = nr.NrProcessor(1, cfg)
    q.process_frames(dx, dy)
    hq = nr.NrProcessor(1, cfg, host=True)
    hy = np.zeros_like(x)
    hq.process_frames(x, hy)
    assert same(dy.cpu().numpy(), hy).all()
    b = nb.NbProcessor(1)
    with pytest.raises(U.UhsdrError) as e:
        b.process_frames(dx, dy, frames=g["frames"] + 1)
    assert e.value.status == U.UHSDR_LENGTH_ERROR
    b.close()
    q.close()
