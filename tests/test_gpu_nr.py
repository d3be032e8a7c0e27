"""Spectral noise reduction on the device (nr_frames and the stream kernels, uhsdr_nr.hip) against
the reference firmware's recorded output (tests/golden/nr_*.npz) with a different case on each
channel, and against the host build of the same step functions on arbitrary seeded input.
Everything is compared exactly (a NaN equals a NaN).  nr_frames runs one wave per channel, four
waves per block: 1, 3, 63, 65 and 130 channels give a partial block, full blocks and a partial
last one.  The calls split the 20-frame start-up inside a call, on a boundary and just after one."""
import ctypes as C

import numpy as np
import pytest

import uhsdr_amd as U
from nr_cases import CASES, FRAME, STREAM_CASES, check_frames, config_of, load_case, load_stream_case
from uhsdr_amd import nr, synth

pytestmark = pytest.mark.gpu

SAME_CONFIG = ("ssb6k_snr10", "restart", "nn_all")          # one configuration, three inputs
RUN = 48                                                    # frames per channel: start-up, then NN varies


def same(a, b):
    """bit for bit, two NaNs equal"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def device_frames(cuda, cfg, rows, frames, sizes, pad=0):
    """rows [C][>= frames * 128] through a device processor in calls of `sizes` frames (cycled; None:
    one call), on rows `pad` floats longer than the run; output [C][frames * 128] and the final state"""
    import torch
    channels, n = rows.shape[0], frames * FRAME
    x = np.zeros((channels, n + pad), np.float32)
    x[:, :n] = rows[:, :n]
    dx = torch.from_numpy(x).to(cuda)
    dy = torch.full_like(dx, 7.0)
    p = nr.NrProcessor(channels, cfg)
    lib, stride = p.lib, n + pad
    at, i = 0, 0
    while at < frames:
        k = frames - at if sizes is None else min(sizes[i % len(sizes)], frames - at)
        U._abi.check(lib.uhsdr_nr_process_frames(p.handle, C.c_void_p(dx.data_ptr() + 4 * at * FRAME),
                                                 C.c_void_p(dy.data_ptr() + 4 * at * FRAME), k, stride), "uhsdr_nr_process_frames")
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
    p = nr.NrProcessor(x.shape[0], cfg, host=True)
    p.process_frames(x, y)
    return y, p.state()


@pytest.mark.parametrize("channels,sizes", [(1, [1]), (3, [19, 1, 28]), (63, [20]), (65, [21]), (130, None), (5, [2]), (6, [3])])
def test_fixtures_one_case_per_channel(cuda, channels, sizes):
    gs = [load_case(n) for n in SAME_CONFIG]
    shift = channels % len(gs)
    mine = [gs[(c + shift) % len(gs)] for c in range(channels)]
    rows = np.stack([g["audio"][:RUN * FRAME] for g in mine])
    cfg = config_of(gs[0])
    y, (ft, nn, ratio) = device_frames(cuda, cfg, rows, RUN, sizes, pad=24)
    for c, g in enumerate(mine):
        upto = RUN if int(g["reset"]) < 0 else int(g["reset"])       # the restart case: up to its restart
        check_frames(g, y[c, :upto * FRAME], what=f"channel {c}")
    hy, (hft, hnn, hratio) = host_frames(cfg, rows, RUN)
    assert same(y, hy).all()
    assert np.array_equal(ft, hft) and (ft == 3).all() and np.array_equal(nn, hnn) and same(ratio, hratio).all()
    for c, g in enumerate(mine):
        if int(g["reset"]) < 0:
            assert nn[c] == g["nn"][RUN - 1], (c, g["name"])


@pytest.mark.parametrize("name", [n for n in CASES if n not in SAME_CONFIG])
def test_other_configurations(cuda, name):
    """every other recorded configuration: the case, its mirror image and a copy 40 dB down"""
    g = load_case(name)
    x = g["audio"][:RUN * FRAME]
    rows = np.stack([x, -x, x * np.float32(0.01)])
    cfg = config_of(g)
    y, state = device_frames(cuda, cfg, rows, RUN, [7, 13, 1])
    check_frames(g, y[0])
    assert np.array_equal(y[1], -y[0])                                              # the chain is odd in its input
    hy, hstate = host_frames(cfg, rows, RUN)
    assert same(y, hy).all()
    assert np.array_equal(state[0], hstate[0]) and np.array_equal(state[1], hstate[1]) and same(state[2], hstate[2]).all()
    assert state[1][0] == g["nn"][RUN - 1]


def test_arbitrary_input_against_the_host_twin(cuda):
    """41 frames over 65 channels: seeded noise at amplitudes from 1e-20 to 1e15, signals in noise, a silent channel
    (0 / 0 in X / xt and in the power ratio), one that falls silent, one with a NaN and one with an
    infinity in it"""
    rng = np.random.default_rng(41)
    channels, frames = 65, 41
    rows = (rng.standard_normal((channels, frames * FRAME)) * 10.0 ** rng.uniform(-20, 15, (channels, 1))).astype(np.float32)
    rows[:8] *= (np.sin(np.arange(frames * FRAME) * 0.3) ** 2).astype(np.float32)      # some with a tone's envelope
    rows[10] = 0.0
    rows[11, 25 * FRAME:] = 0.0
    rows[12, 30 * FRAME + 5] = np.nan
    rows[13, 22 * FRAME + 77] = np.inf
    for k in range(24):                                     # voiced and keyed signals from -3 to 20 dB SNR: NN varies
        rows[20 + k] = synth.nr_audio(frames * FRAME, rate=6000.0, snr_db=-3.0 + k, seed=k, amplitude=3000.0 / (1 + k % 5))
    for kw in (dict(), dict(width_hz=200, offset_hz=400, nr_strength=1, asnr=15), dict(width_hz=3200, offset_hz=1700, sample_rate=12000, width=5)):
        cfg = nr.nr_config(**kw)
        y, state = device_frames(cuda, cfg, rows, frames, [5, 16])
        hy, hstate = host_frames(cfg, rows, frames)
        bad = np.argwhere(~same(y, hy))
        assert len(bad) == 0, (kw, "first difference at channel, sample", bad[0].tolist(), "of", len(bad))
        assert np.array_equal(state[0], hstate[0]) and np.array_equal(state[1], hstate[1]) and same(state[2], hstate[2]).all()
        assert np.isnan(state[2][10]) and state[1][10] == 1                            # the silent channel: NN = 1
        assert len(set(state[1].tolist())) > 2


def device_stream(cuda, cfg, rows, calls):
    """rows [C][n] through uhsdr_nr_process in calls of the given sizes, the rows staying on the device"""
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
    state = p.state()
    p.close()
    return y, state


def host_stream(cfg, rows):
    y = np.zeros_like(rows)
    p = nr.NrProcessor(rows.shape[0], cfg, host=True)
    p.process(np.ascontiguousarray(rows), y)
    return y, p.state()


@pytest.mark.parametrize("name", STREAM_CASES)
def test_stream_in_calls_of_8(cuda, name):
    """600 calls of 8 samples at 65 channels: channel 0 the recorded case, the others scaled copies"""
    g = load_stream_case(name)
    n = 600 * 8
    gains = (10.0 ** np.linspace(0.0, -3.0, 65)).astype(np.float32)
    rows = g["audio"][None, :n] * gains[:, None]
    cfg = config_of(g)
    y, state = device_stream(cuda, cfg, rows, [8] * 600)
    assert np.array_equal(y[0].view(np.uint32), g["out"][:n].view(np.uint32))
    hy, hstate = host_stream(cfg, rows)
    assert same(y, hy).all()
    assert np.array_equal(state[0], hstate[0]) and np.array_equal(state[1], hstate[1])


@pytest.mark.parametrize("name", STREAM_CASES)
def test_stream_in_one_large_call(cuda, name):
    """one 4000-sample call, then the rest in calls that grow and shrink the work rows"""
    g = load_stream_case(name)
    x = g["audio"]
    rows = np.stack([x, -x, x[::-1]])
    y, state = device_stream(cuda, config_of(g), rows, [4000, 8, 3000, 992])
    assert np.array_equal(y[0].view(np.uint32), g["out"].view(np.uint32))
    hy, hstate = host_stream(config_of(g), rows)
    assert same(y, hy).all() and np.array_equal(state[1], hstate[1])


def test_reset_and_refusals_on_the_device(cuda):
    import torch
    g = load_case("cw6k_snr5")
    x = np.array(g["audio"][None, :RUN * FRAME])            # a writable copy for torch
    dx = torch.from_numpy(x).to(cuda)
    dy = torch.zeros_like(dx)
    p = nr.NrProcessor(1, config_of(g))
    p.process_frames(dx, dy, frames=30)
    p.reset()
    assert p.state()[0][0] == 1
    p.process_frames(dx, dy)
    check_frames(g, dy.cpu().numpy()[0])
    with pytest.raises(U.UhsdrError) as e:
        p.process_frames(dx, dy, frames=RUN + 1)
    assert e.value.status == U.UHSDR_LENGTH_ERROR
    with pytest.raises(U.UhsdrError) as e:
        p.process(dx, dy, n=12)
    assert e.value.status == U.UHSDR_LENGTH_ERROR
    p.close()
