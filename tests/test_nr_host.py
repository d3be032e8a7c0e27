"""Spectral noise reduction on the CPU (uhsdr_nr_process_frames_host / uhsdr_nr_process_host: the
step functions the nr_frames kernel runs) against what the reference firmware computed
(tests/golden/nr_*.npz, recorded by tools/nr/make_nr_golden.py).  Everything is exact: the bits of
every output sample and NN of every frame."""
import ctypes as C

import numpy as np
import pytest

import uhsdr_amd as U
from uhsdr_amd import _abi, nr

from nr_cases import CASES, FRAME, SHOW, STREAM_CASES, check_frames, config_of, load_case, load_stream_case

# calls in frames: the switch first_time 2 -> 3 (frame 19) inside a call, on a boundary, just after one
SPLITS = {"whole": None, "1": [1], "2": [2], "3": [3], "19+1": [19, 1], "20": [20], "21": [21]}


def run_frames(g, sizes, proc=None, first=0, last=None):
    """the frames first .. last of a case in calls of `sizes` frames (cycled); output and per-frame NN"""
    p = proc or nr.NrProcessor(1, config_of(g), host=True)
    last = g["frames"] if last is None else last
    y = np.zeros((last - first) * FRAME, np.float32)
    nn = np.zeros(last - first, np.int32)
    at, i = first, 0
    while at < last:
        k = last - at if sizes is None else min(sizes[i % len(sizes)], last - at)
        x = np.ascontiguousarray(g["audio"][at * FRAME:(at + k) * FRAME]).reshape(1, -1)
        out = np.zeros_like(x)
        p.process_frames(x, out)
        y[(at - first) * FRAME:(at - first + k) * FRAME] = out[0]
        nn[at - first:at - first + k] = -1                          # only the call's last frame shows its NN
        nn[at - first + k - 1] = p.state()[1][0]
        at += k
        i += 1
    return p, y, nn


def test_fixture_set_covers_the_noise_reduction():
    assert set(CASES) == set(SHOW)
    gs = {n: load_case(n) for n in CASES}                   # (the loader asserts what each recording shows)
    assert {g["cfg"]["sample_rate"] for g in gs.values()} == {6000, 12000}
    assert {g["cfg"]["asnr"] for g in gs.values()} >= {15, 30}
    lib = U.load()
    alphas = {np.float32(g["cfg"]["alpha"]) for g in gs.values()}
    assert {np.float32(lib.uhsdr_nr_alpha_from_strength(s)) for s in (1, 200)} <= alphas
    snr = [g["gen"] for g in gs.values()]
    assert any('"snr_db": -3.0' in str(s) for s in snr) and any('"snr_db": 20.0' in str(s) for s in snr)
    assert set(STREAM_CASES) == {"ssb", "cw", "wide"}


@pytest.mark.parametrize("name", [n for n in CASES if n != "nn_all"])       # (the 400-frame case runs in test_call_splits)
def test_case_frame_by_frame(name):
    """one frame a call: every output bit, and NN, power_ratio and first_time of every frame"""
    g = load_case(name)
    reset = int(g["reset"])
    p = nr.NrProcessor(1, config_of(g), host=True)
    y = np.zeros((g["frames"], FRAME), np.float32)
    for f in range(g["frames"]):
        if f == reset:
            p.reset()
        x = np.ascontiguousarray(g["audio"][f * FRAME:(f + 1) * FRAME]).reshape(1, -1)
        out = np.zeros_like(x)
        p.process_frames(x, out)
        y[f] = out[0]
        ft, nn, ratio = p.state()
        assert ft[0] == g["first_time"][f], (name, f)
        if g["running"][f]:
            assert nn[0] == g["nn"][f], (name, f)
            want = g["power_ratio"][f]                       # NaN for a band without power: any NaN
            assert (np.isnan(ratio[0]) and np.isnan(want)) or ratio.view(np.uint32)[0] == want.view(np.uint32), (name, f)
    check_frames(g, y)


@pytest.mark.parametrize("split", list(SPLITS))
def test_call_splits(split):
    for name in ("ssb6k_snr10", "cw6k_snr5", "wide12k_snrm3", "nn_all"):
        g = load_case(name)
        p, y, nn = run_frames(g, SPLITS[split])
        check_frames(g, y, what=split)
        seen = nn >= 0
        seen &= g["running"]
        assert np.array_equal(nn[seen], g["nn"][seen]), (name, split)
        assert p.state()[0][0] == 3


def test_restart_and_reset_reproduce_the_run():
    g = load_case("restart")
    reset = int(g["reset"])
    p, y0, _ = run_frames(g, [7], last=reset)
    p.reset()
    _, y1, _ = run_frames(g, [5], proc=p, first=reset)
    check_frames(g, np.concatenate([y0, y1]))
    # the same processor after a reset computes the same run again
    g = load_case("ssb6k_snr3_asnr15")
    p, y, _ = run_frames(g, None)
    p.reset()
    _, again, _ = run_frames(g, [4], proc=p)
    assert np.array_equal(y.view(np.uint32), again.view(np.uint32))
    check_frames(g, again)


def test_channels_are_independent():
    gs = [load_case(n) for n in ("ssb6k_snr10", "ssb6k_snr3_asnr15")]       # one configuration apart from asnr
    g = gs[0]
    rows = np.stack([g["audio"], gs[1]["audio"], g["audio"][::-1]]).astype(np.float32)
    pad = np.zeros((3, rows.shape[1] + 40), np.float32)                    # stride > n
    pad[:, :rows.shape[1]] = rows
    out = np.full_like(pad, 7.0)
    p = nr.NrProcessor(3, config_of(g), host=True)
    p.process_frames(pad, out, frames=g["frames"])
    check_frames(g, out[0, :rows.shape[1]])
    assert (out[:, rows.shape[1]:] == 7.0).all()
    assert not np.array_equal(out[0], out[2])


@pytest.mark.parametrize("name", STREAM_CASES)
@pytest.mark.parametrize("call", [8, 24, 136, 1000, None])
def test_stream(name, call):
    g = load_stream_case(name)
    x = g["audio"]
    p = nr.NrProcessor(2, config_of(g), host=True)
    y = np.zeros((2, len(x)), np.float32)
    step = call or len(x)
    for s in range(0, len(x), step):
        n = min(step, len(x) - s)
        a = np.ascontiguousarray(np.stack([x[s:s + n], -x[s:s + n]]))
        b = np.zeros_like(a)
        p.process(a, b)
        y[:, s:s + n] = b
    bad = np.flatnonzero(y[0].view(np.uint32) != g["out"].view(np.uint32))
    assert len(bad) == 0, (name, call, "first differing sample", int(bad[0]), "of", len(bad))
    assert y[1].any() and not np.array_equal(y[0], y[1])
    # a reset starts the stream again: the FIFO is silent for two frames and the same output follows
    p.reset()
    a = np.ascontiguousarray(np.stack([x[:2000], -x[:2000]]))
    b = np.zeros_like(a)
    p.process(a, b)
    assert np.array_equal(b[0].view(np.uint32), g["out"][:2000].view(np.uint32))


def test_refused_configurations():
    lib = U.load()
    h = C.c_void_p()
    ok = nr.nr_config()
    assert lib.uhsdr_nr_create_host(1, C.byref(ok), C.byref(h)) == _abi.UHSDR_OK
    x = np.zeros((1, 256), np.float32)
    px = x.ctypes.data_as(C.c_void_p)
    assert lib.uhsdr_nr_process_frames_host(h, px, px, 3, 256) == _abi.UHSDR_LENGTH_ERROR      # 3 frames do not fit
    assert lib.uhsdr_nr_process_host(h, px, px, 12, 256) == _abi.UHSDR_LENGTH_ERROR            # not a multiple of 8
    assert lib.uhsdr_nr_process_host(h, px, px, 264, 256) == _abi.UHSDR_LENGTH_ERROR
    assert lib.uhsdr_nr_process_frames(h, px, px, 1, 256) == _abi.UHSDR_ARGUMENT_ERROR         # a host handle
    assert lib.uhsdr_nr_process_frames_host(h, None, px, 1, 256) == _abi.UHSDR_ARGUMENT_ERROR
    lib.uhsdr_nr_destroy(h)
    bad = [dict(alpha=1.5), dict(alpha=float("nan")), dict(asnr=1), dict(asnr=31), dict(width=0), dict(width=6),
           dict(power_threshold_int=9), dict(power_threshold_int=101), dict(sample_rate=8000), dict(width_hz=-1),
           dict(offset_hz=70000)]
    # bands the reference's smoothing loops would leave their arrays with (width 4: NN up to 9):
    # VAD_high below 17, VAD_low above 116 with a band that is not empty
    bad += [dict(width_hz=200, offset_hz=250), dict(width_hz=200, offset_hz=400, sample_rate=12000),
            dict(width_hz=200, offset_hz=2850), dict(width_hz=300, offset_hz=5700, sample_rate=12000)]
    for kw in bad:
        assert lib.uhsdr_nr_create_host(1, C.byref(nr.nr_config(**kw)), C.byref(h)) == _abi.UHSDR_ARGUMENT_ERROR, kw
    assert lib.uhsdr_nr_create_host(0, C.byref(ok), C.byref(h)) == _abi.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_nr_create_host(1, None, C.byref(h)) == _abi.UHSDR_ARGUMENT_ERROR
    # the edges of the accepted region for width 4, and what width 5 moves them to
    assert nr.nr_band(nr.nr_config(width_hz=200, offset_hz=300)) == (8, 17)
    assert nr.nr_band(nr.nr_config(width_hz=200, offset_hz=2830)) == (116, 125)
    assert lib.uhsdr_nr_band(C.byref(nr.nr_config(width_hz=200, offset_hz=300, width=5)), None, None) == _abi.UHSDR_ARGUMENT_ERROR
    assert nr.nr_band(nr.nr_config(width_hz=200, offset_hz=400, width=5)) == (12, 21)
    # a stream whose band is only valid at the other rate is refused by process, not by create
    p = nr.NrProcessor(1, nr.nr_config(width_hz=3600, offset_hz=2000, sample_rate=6000), host=True)
    assert nr.nr_band(p.cfg) == (8, 128)
    x8 = np.zeros((1, 8), np.float32)
    p.process(x8, np.zeros_like(x8))                          # 12 ksps frames: bins (4, 81), accepted
    q = nr.NrProcessor(1, nr.nr_config(width_hz=2800, offset_hz=7000, sample_rate=6000), host=True)
    assert nr.nr_band(q.cfg) == (126, 102)                    # 6 ksps frames: an empty band, accepted
    with pytest.raises(U.UhsdrError) as e:
        q.process(x8, np.zeros_like(x8))                      # 12 ksps frames: bins (119, 128), VAD_low above 116
    assert e.value.status == _abi.UHSDR_ARGUMENT_ERROR
