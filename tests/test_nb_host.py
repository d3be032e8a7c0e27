"""Noise blanker on the CPU (uhsdr_nb_process_frames_host and the stream's uhsdr_nr_process_host with
the blanker in it: the step functions the nb_frames kernel runs) against what the reference firmware
computed (tests/golden/nb_*.npz, recorded by tools/nb/make_nb_golden.py).  Everything is exact: the
bits of every output sample (a NaN equals a NaN)."""
import ctypes as C

import numpy as np
import pytest

import uhsdr_amd as U
from uhsdr_amd import _abi, nb, nr

import nr_cases
from nb_cases import (CASES, FRAME, SHOW, STREAM_CASES, STREAM_SHOW, check_frames, check_sparse_grows, config_of, load_case, load_stream_case,
                      same, stream_config_of)


def run_frames(g, size, in_place=False, proc=None):
    """a case in calls of `size` frames (None: one call); the processor and the output"""
    p = proc or nb.NbProcessor(1, config_of(g), host=True)
    y = np.zeros(g["frames"] * FRAME, np.float32)
    size = size or g["frames"]
    for at in range(0, g["frames"], size):
        k = min(size, g["frames"] - at)
        x = np.array(g["audio"][at * FRAME:(at + k) * FRAME]).reshape(1, -1)
        if in_place:
            p.process_frames(x)
            y[at * FRAME:(at + k) * FRAME] = x[0]
        else:
            out = np.zeros_like(x)
            p.process_frames(x, out)
            y[at * FRAME:(at + k) * FRAME] = out[0]
    return p, y


def test_fixture_set_covers_the_blanker():
    assert set(CASES) == set(SHOW) and set(STREAM_CASES) == set(STREAM_SHOW)
    for n in CASES:
        load_case(n)                                        # (the loader asserts what each recording shows)
    for n in STREAM_CASES:
        load_stream_case(n)
    check_sparse_grows()
    assert {s for s, _ in SHOW.values()} == {1, 8, 15}


@pytest.mark.parametrize("name", sorted(SHOW))
@pytest.mark.parametrize("size,in_place", [(1, False), (7, False), (None, False), (None, True), (7, True)])
def test_case(name, size, in_place):
    g = load_case(name)
    p, y = run_frames(g, size, in_place)
    check_frames(g, y, what=(size, in_place))


@pytest.mark.parametrize("name", sorted(SHOW))
def test_state_counts_the_repairs(name):
    """total_count > 0 exactly where the recording shows changes; every repair is seven samples"""
    g = load_case(name)
    p = nb.NbProcessor(1, config_of(g), host=True)
    total_before = 0
    for f in range(g["frames"]):
        x = np.array(g["audio"][f * FRAME:(f + 1) * FRAME]).reshape(1, -1)
        p.process_frames(x)
        last, total = p.state()
        assert 0 <= last[0] <= nb.MAX_HITS and total[0] == total_before + last[0], (name, f)
        total_before = int(total[0])
    changes = int(g["changed"].sum())
    assert (total_before > 0) == (changes > 0), name
    assert nb.REPAIR * total_before >= changes, name
    if SHOW[name][1] == "burst":
        assert total_before == nb.MAX_HITS                  # eight impulses in one frame, 35 samples changed: the cap


def test_reset_reproduces_the_run():
    g = load_case("walk")
    p, y = run_frames(g, 5)
    assert p.state()[1][0] > 0
    p.reset()
    assert p.state()[0][0] == 0 and p.state()[1][0] == 0
    _, again = run_frames(g, None, proc=p)
    check_frames(g, again)
    assert same(y, again).all()


def test_channels_are_independent_and_rows_are_respected():
    gs = [load_case(n) for n in ("sparse_s8", "burst8", "walk")]
    n = gs[0]["frames"] * FRAME
    pad = np.zeros((3, n + 24), np.float32)
    for c, g in enumerate(gs):
        pad[c, :n] = g["audio"]
    out = np.full_like(pad, 7.0)
    p = nb.NbProcessor(3, config_of(gs[0]), host=True)
    p.process_frames(pad, out, frames=gs[0]["frames"])
    for c, g in enumerate(gs):
        check_frames(g, out[c, :n], what=f"channel {c}")
    assert (out[:, n:] == 7.0).all()


def stream_run(cfg, rows, calls):
    p = nr.NrProcessor(rows.shape[0], cfg, host=True)
    y = np.zeros_like(rows)
    at = 0
    for k in calls:
        a = np.ascontiguousarray(rows[:, at:at + k])
        b = np.zeros_like(a)
        p.process(a, b)
        y[:, at:at + k] = b
        at += k
    assert at == rows.shape[1]
    return p, y


@pytest.mark.parametrize("name", sorted(STREAM_SHOW))
@pytest.mark.parametrize("calls", ["8", "large"])
def test_stream(name, calls):
    g = load_stream_case(name)
    x = g["audio"]
    rows = np.stack([x, -x])
    p, y = stream_run(stream_config_of(g), rows, [8] * 600 if calls == "8" else [4000, 8, 792])
    bad = np.flatnonzero(~same(y[0], g["out"]))
    assert len(bad) == 0, (name, calls, "first differing sample", int(bad[0]), "of", len(bad))
    assert y[1].any()
    # a reset starts the stream and the blanker again
    p.reset()
    a = np.ascontiguousarray(rows[:, :2000])
    b = np.zeros_like(a)
    p.process(a, b)
    assert same(b[0], g["out"][:2000]).all()


@pytest.mark.parametrize("name", nr_cases.STREAM_CASES)
def test_stream_without_the_blanker_is_unchanged(name):
    """nb_setting 0 and nr_bypass 0, the defaults: the bytes of the existing recordings"""
    g = nr_cases.load_stream_case(name)
    cfg = nr_cases.config_of(g)
    assert cfg.nb_setting == 0 and cfg.nr_bypass == 0
    x = g["audio"][:4800]
    p, y = stream_run(cfg, np.stack([x, -x]), [8] * 600)
    assert np.array_equal(y[0].view(np.uint32), g["out"][:4800].view(np.uint32))


def test_frames_through_the_noise_reduction_handle():
    """uhsdr_nr_process_frames_host honours both fields: the blanker alone gives the blanker's
    recording; the blanker in front of the noise reduction gives what the two handles give in turn"""
    g = load_case("sparse_s8")
    x = np.array(g["audio"]).reshape(1, -1)
    p = nr.NrProcessor(1, nr.nr_config(nb_setting=8, nr_bypass=1, sample_rate=12000, width_hz=3200, offset_hz=1700), host=True)
    y = np.zeros_like(x)
    p.process_frames(x, y)
    check_frames(g, y[0])
    both = nr.NrProcessor(1, nr.nr_config(nb_setting=8, sample_rate=12000, width_hz=3200, offset_hz=1700), host=True)
    z = np.zeros_like(x)
    both.process_frames(x, z)
    alone = nr.NrProcessor(1, nr.nr_config(sample_rate=12000, width_hz=3200, offset_hz=1700), host=True)
    want = np.zeros_like(x)
    alone.process_frames(np.ascontiguousarray(y), want)
    assert same(z, want).all() and not same(z, y).all()


def test_refusals():
    lib = U.load()
    h = C.c_void_p()

    def refused(call, status, text):
        assert call == status
        assert lib.uhsdr_last_error().decode() == text

    for bad in (0, -1, 16):
        refused(lib.uhsdr_nb_create_host(1, C.byref(nb.nb_config(nb_setting=bad)), C.byref(h)), _abi.UHSDR_ARGUMENT_ERROR,
                f"nb: nb_setting {bad} outside 1..15")
    refused(lib.uhsdr_nb_create_host(0, C.byref(nb.nb_config()), C.byref(h)), _abi.UHSDR_ARGUMENT_ERROR, "nb: bad argument")
    refused(lib.uhsdr_nb_create_host(1, None, C.byref(h)), _abi.UHSDR_ARGUMENT_ERROR, "nb: bad argument")
    assert nb.nb_config().nb_setting == 8
    for s in (1, 15):
        assert lib.uhsdr_nb_create_host(1, C.byref(nb.nb_config(nb_setting=s)), C.byref(h)) == _abi.UHSDR_OK
        x = np.zeros((1, 256), np.float32)
        px = x.ctypes.data_as(C.c_void_p)
        refused(lib.uhsdr_nb_process_frames_host(h, px, px, 3, 256), _abi.UHSDR_LENGTH_ERROR, "nb: 3 frames of 128 samples do not fit a row of 256")
        refused(lib.uhsdr_nb_process_frames_host(h, px, px, -1, 256), _abi.UHSDR_LENGTH_ERROR, "nb: -1 frames of 128 samples do not fit a row of 256")
        refused(lib.uhsdr_nb_process_frames_host(h, None, px, 1, 256), _abi.UHSDR_ARGUMENT_ERROR, "null argument")
        refused(lib.uhsdr_nb_process_frames(h, px, px, 1, 256), _abi.UHSDR_ARGUMENT_ERROR, "nb: host handle, use uhsdr_nb_process_frames_host")
        refused(lib.uhsdr_nb_set_stream(h, None), _abi.UHSDR_ARGUMENT_ERROR, "nb: not a device handle")
        assert lib.uhsdr_nb_process_frames_host(h, px, px, 0, 256) == _abi.UHSDR_OK
        assert lib.uhsdr_nb_process_frames_host(h, px, px, 2, 256) == _abi.UHSDR_OK
        lib.uhsdr_nb_destroy(h)
    refused(lib.uhsdr_nb_state(None, None, None), _abi.UHSDR_ARGUMENT_ERROR, "null handle")
    # the two fields of the noise reduction's configuration
    assert nr.nr_config().nb_setting == 0 and nr.nr_config().nr_bypass == 0 and C.sizeof(_abi.NrConfig) == 64
    refused(lib.uhsdr_nr_create_host(1, C.byref(nr.nr_config(nr_bypass=1)), C.byref(h)), _abi.UHSDR_ARGUMENT_ERROR,
            "nr: nr_bypass without the noise blanker (nb_setting 0): the firmware does not enter the stream then")
    refused(lib.uhsdr_nr_create_host(1, C.byref(nr.nr_config(nb_setting=16)), C.byref(h)), _abi.UHSDR_ARGUMENT_ERROR, "nr: nb_setting 16 outside 0..15")
    refused(lib.uhsdr_nr_create_host(1, C.byref(nr.nr_config(nb_setting=-1)), C.byref(h)), _abi.UHSDR_ARGUMENT_ERROR, "nr: nb_setting -1 outside 0..15")
    refused(lib.uhsdr_nr_create_host(1, C.byref(nr.nr_config(nb_setting=3, nr_bypass=2)), C.byref(h)), _abi.UHSDR_ARGUMENT_ERROR, "nr: nr_bypass 2: 0 or 1")
