"""The waterfall image's host side against the reference firmware's recordings (tests/wfall_cases.py):
the host twin (uhsdr_wfall_process_lines_host runs the step functions the kernels run, frame after
frame as the firmware does), the plan, the counters, the refusals, and the generated palette header.
No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import uhsdr_amd as U
import wfall_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def new_host(g, **over):
    return U.Waterfall(g["channels"], wc.config_of(g, **over), host=True)


def sentinel(g):
    return np.full((g["channels"], g["H"], g["W"]), wc.SENTINEL, np.uint16)


def run_calls(g, w, step, center=True):
    """the case in calls of `step` frames on one image, checked after every call"""
    image = sentinel(g)
    for first in range(0, g["frames"], step):
        n = min(step, g["frames"] - first)
        hz = np.ascontiguousarray(g["center_hz"][:, first:first + n]) if center else None
        got = w.process_lines_host(np.ascontiguousarray(g["lines"][:, first:first + n]), hz, image)
        assert (got["drawn"] == g["drawn"][:, first:first + n]).all(), (g["name"], first)
        wc.check_image(g, image, first + n - 1, f"host, calls of {step}")
    return image


def test_the_set_shows_what_it_must():
    assert len(wc.CASES) >= 34 and wc.SPEC_CASE in wc.CASES
    assert not (wc.palettes() == wc.SENTINEL).any()
    wc.check_set()


@pytest.mark.parametrize("name", wc.CASES)
def test_host_twin_matches_reference_firmware_frame_by_frame(name):
    g = wc.load_case(name)
    w = new_host(g)
    run_calls(g, w, 1)
    st = w.state()
    # sd.wfall_line is reduced at the start of the next frame (:1101): compared modulo the ring
    assert st["wfall_line"] % w.plan.wfall_size == int(g["counters"][0]) % w.plan.wfall_size
    assert st["wfall_line_update"] == int(g["counters"][1])


@pytest.mark.parametrize("name", wc.CASES)
def test_call_granularity(name):
    """all frames in one call, and calls of three, leave what the frame-by-frame calls leave"""
    g = wc.load_case(name)
    for step in (g["frames"], 3):
        run_calls(g, new_host(g), step)


@pytest.mark.parametrize("name", wc.CASES)
def test_plan_matches_the_firmwares_values(name):
    g = wc.load_case(name)
    p = U.wfall_plan(wc.config_of(g))
    assert (p.wfall_size, p.repeat, p.marker_num) == tuple(int(v) for v in g["plan_ints"])
    got = np.array([p.hz_per_pixel, p.rx_carrier_pos, *p.marker_pos], np.float32)
    assert got.tobytes() == g["plan_floats"].tobytes(), (got, g["plan_floats"])
    assert (np.array(p.colours[:], np.uint16) == g["colours"]).all()
    # the firmware's conversion of marker_pos to uint16_t on x86: truncated to int32, the low 16 bits
    for m in range(p.marker_num):
        assert p.marker_pixel[m] == int(np.int32(np.trunc(g["plan_floats"][2 + m]))) & 0xFFFF
    for m in range(p.marker_num, 3):
        assert p.marker_pixel[m] == p.width and p.marker_pos[m] == p.width
    assert (p.width, p.height, p.vert_step_size) == (g["W"], g["H"], g["cfg"]["vert_step_size"])


def test_plan_of_the_default_configuration_and_the_ring_sizes():
    p = U.wfall_plan(U.wfall_config())
    assert (p.width, p.height, p.wfall_size, p.repeat, p.vert_step_size, p.marker_num) == (256, 70, 70, 1, 2, 1)
    assert p.hz_per_pixel == np.float32(187.5) and p.rx_carrier_pos == np.float32(127.5 + 64) and p.colours[64] == 0xFFFF
    for (W, H), want in {(480, 70): (35, 2), (512, 40): (40, 1), (512, 41): (20, 2), (512, 81): (40, 2), (512, 255): (40, 6),
                         (128, 80): (80, 1), (256, 160): (80, 2), (256, 255): (80, 3), (300, 137): (68, 2)}.items():
        p = U.wfall_plan(U.wfall_config(width=W, height=H))
        assert (p.wfall_size, p.repeat) == want, (W, H)
    assert U.load().uhsdr_sizeof_wfall_config() == C.sizeof(U.WfallConfig)
    assert U.load().uhsdr_sizeof_wfall_plan() == C.sizeof(U.WfallPlan)


def test_counters_replay_of_the_firmwares_lines():
    """the ring line every frame writes is the firmware's (`at` of the recording), through the ring's wrap"""
    for name in ("wrap", "step2", "panel", "memlimit", "shift_m3"):
        g = wc.load_case(name)
        w = new_host(g)
        for f in range(g["frames"]):
            st = w.state()
            assert st["wfall_line"] % w.plan.wfall_size == int(g["at"][f]), (name, f)
            w.process_lines_host(np.ascontiguousarray(g["lines"][:, f:f + 1]))


@pytest.mark.parametrize("bad", [
    dict(width=127), dict(width=513), dict(height=0), dict(height=256), dict(color_scheme=-1), dict(color_scheme=5),
    dict(vert_step_size=0), dict(vert_step_size=6), dict(marker_colour=-1), dict(marker_colour=65536), dict(magnify=-1), dict(magnify=6),
    dict(iq_freq_mode=-1), dict(iq_freq_mode=5), dict(dmod_mode=-1), dict(dmod_mode=9), dict(digital_mode=-1), dict(digital_mode=3),
    dict(cw_lsb=2), dict(digi_lsb=-1), dict(cw_sidetone_freq=-1), dict(cw_sidetone_freq=65536), dict(rtty_shift_idx=-1),
    dict(rtty_shift_idx=6), dict(psk_speed_idx=-1), dict(psk_speed_idx=3),
    dict(width=128, height=81), dict(width=128, height=255), dict(width=200, height=190),     # more ring lines than the firmware has frequencies
], ids=str)
def test_refusals(bad):
    lib = U.load()
    cfg = U.wfall_config(**bad)
    plan = U.WfallPlan()
    assert lib.uhsdr_wfall_plan_build(C.byref(cfg), C.byref(plan)) == U.UHSDR_ARGUMENT_ERROR
    assert b"wfall" in lib.uhsdr_last_error()
    h = C.c_void_p()
    assert lib.uhsdr_wfall_create_host(2, C.byref(cfg), C.byref(h)) == U.UHSDR_ARGUMENT_ERROR and not h.value


def test_aliasing_wrong_kind_and_null_arguments():
    lib = U.load()
    w = U.Waterfall(2, U.wfall_config(width=128, height=4), host=True)
    lines = np.zeros((2, 8, 128), np.uint8)
    p = lines.ctypes.data_as(C.c_void_p)
    # image inside the lines, at their start and at their last byte pair
    for at in (0, lines.nbytes - 2):
        io = U.WfallIo(image=lines.ctypes.data + at)
        assert lib.uhsdr_wfall_process_lines_host(w.handle, p, None, 8, C.byref(io)) == U.UHSDR_ARGUMENT_ERROR
        assert b"overlap" in lib.uhsdr_last_error()
    # lines inside the image
    image = np.zeros((2, 4, 128), np.uint16)
    io = U.WfallIo(image=image.ctypes.data)
    assert lib.uhsdr_wfall_process_lines_host(w.handle, C.c_void_p(image.ctypes.data + 64), None, 1, C.byref(io)) == U.UHSDR_ARGUMENT_ERROR
    io = U.WfallIo(image=image.ctypes.data + 1)
    assert lib.uhsdr_wfall_process_lines_host(w.handle, p, None, 8, C.byref(io)) == U.UHSDR_ARGUMENT_ERROR
    assert w.state() == dict(wfall_line=0, double_line_start=0, wfall_line_update=0)       # a refused call moves nothing
    assert lib.uhsdr_wfall_process_lines(w.handle, p, None, 8, None) == U.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_wfall_process_lines_host(w.handle, None, None, 1, None) == U.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_wfall_process_lines_host(w.handle, p, None, -1, None) == U.UHSDR_LENGTH_ERROR
    assert lib.uhsdr_wfall_set_stream(w.handle, None) == U.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_wfall_create_host(0, C.byref(w.cfg), C.byref(C.c_void_p())) == U.UHSDR_ARGUMENT_ERROR
    with pytest.raises(ValueError):
        w.process_lines(lines)
    with pytest.raises(ValueError):
        w.process_lines_host(np.zeros((2, 1, 129), np.uint8))


def test_state_reset_and_null_io():
    g = wc.load_case("step2")
    w = new_host(g)
    assert w.state() == dict(wfall_line=0, double_line_start=0, wfall_line_update=0)
    lines = np.ascontiguousarray(g["lines"][:, :5])
    w._call("process_lines_host", lines.ctypes.data_as(C.c_void_p), None, 5, None)          # ring and counters only
    image = sentinel(g)
    got = w.process_lines_host(np.ascontiguousarray(g["lines"][:, 5:]), None, image)
    assert (got["drawn"] == g["drawn"][:, 5:]).all()
    wc.check_image(g, image, g["frames"] - 1, "behind a call without io")
    assert w.state()["wfall_line_update"] == int(g["counters"][1])
    w.reset()
    assert w.state() == dict(wfall_line=0, double_line_start=0, wfall_line_update=0)
    run_calls(g, w, 1)


def test_doubleLineStart_is_zero_after_reset():
    """defined here: the firmware's function static is never cleared; a reset after an odd number of frames (repeat 1
    leaves it at 1) starts over like a new handle"""
    g = wc.load_case("w200_h9")
    w = new_host(g)
    w.process_lines_host(np.ascontiguousarray(g["lines"][:, :3]))
    assert w.state()["double_line_start"] == 1
    w.reset()
    run_calls(g, w, 2)


def test_null_center_is_every_frame_at_zero():
    g = wc.load_case("pal1")
    assert (g["center_hz"] == 0).all()
    run_calls(g, new_host(g), 2, center=False)
    # and a case with shifts, run without them, shows no padding: no black but what the palette's entries give
    g = wc.load_case("far_below")
    w = new_host(g)
    got = w.process_lines_host(g["lines"])
    body = got["image"][:, :, [0, -1]]
    assert (body != 0).all()


def test_a_byte_above_64_is_colour_0_and_64_the_markers():
    cfg = U.wfall_config(width=128, height=2, color_scheme=4, marker_colour=0x1234, vert_step_size=1, iq_freq_mode=0)
    w = U.Waterfall(1, cfg, host=True)
    lines = np.zeros((1, 2, 128), np.uint8)
    lines[0, :, :8] = (63, 64, 65, 100, 128, 200, 254, 255)
    got = w.process_lines_host(lines)["image"][0]
    pal = wc.palettes()[4]
    assert pal[0] != 0
    assert got[0, :8].tolist() == [pal[63], 0x1234] + [pal[0]] * 6
    assert got[0, 63] == 0x1234 and got[0, 62] == pal[0]          # the marker at the carrier, (uint16_t)63.5


def test_table_header_is_what_the_fixture_gives():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "wfall", "gen_wfall_tables.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
