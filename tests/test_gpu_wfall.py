"""The waterfall image on the device against the reference firmware's recordings (tests/wfall_cases.py):
wfall_image and wfall_commit on every case, frame by frame and in one call; calls that draw not at
all, once and several times; a call longer than the ring; 130 channels with another case in every
neighbouring channel and four widths against the host twin; optional outputs and sentinels; reset; a
null centre-frequency row; and the stage chained behind Display.process_avg on one stream.  Bit for
bit on every pixel."""
import json
import os

import numpy as np
import pytest

import display_cases as dc
import uhsdr_amd as U
import wfall_cases as wc

pytestmark = pytest.mark.gpu

IMAGE_SENTINEL = wc.SENTINEL - 65536        # the same two bytes in an int16 tensor
DRAWN_SENTINEL = 0x77


def device_outputs(w, F):
    import torch
    return dict(image=torch.full(w.output_shape("image", F), IMAGE_SENTINEL, dtype=torch.int16, device="cuda"),
                drawn=torch.full(w.output_shape("drawn", F), DRAWN_SENTINEL, dtype=torch.uint8, device="cuda"))


def image_of(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint16)


def put(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype) if dtype is not None else a).cuda()


def run_calls(g, w, step, center=True):
    """the case in calls of `step` frames on one image, image and drawn checked after every call"""
    out = device_outputs(w, 0)
    for first in range(0, g["frames"], step):
        n = min(step, g["frames"] - first)
        drawn = device_outputs(w, n)["drawn"]
        w.process_lines(put(g["lines"][:, first:first + n]), put(g["center_hz"][:, first:first + n], np.int32) if center else None,
                        image=out["image"], drawn=drawn)
        w.synchronize()
        assert (drawn.cpu().numpy() == g["drawn"][:, first:first + n]).all(), (g["name"], first)
        wc.check_image(g, image_of(out["image"]), first + n - 1, f"device, calls of {step}")


@pytest.mark.parametrize("name", wc.CASES)
def test_frame_by_frame_and_in_one_call_matches_reference_firmware(cuda, name):
    g = wc.load_case(name)
    run_calls(g, U.Waterfall(g["channels"], wc.config_of(g)), 1)
    run_calls(g, U.Waterfall(g["channels"], wc.config_of(g)), g["frames"])


@pytest.mark.parametrize("name,step", [("step5", 2), ("step5", 5), ("step5", 13), ("step2", 3), ("wrap", 7), ("wrap", 15), ("shift_m4", 6),
                                       ("panel", 2), ("memlimit", 4)])
def test_call_sizes(cuda, name, step):
    """step5 in calls of 2 draws in none of the first two calls, in calls of 5 once a call, in calls of 13 twice in the
    first; wrap's ring has three lines, so a call of 7 or 15 frames overwrites lines earlier frames of the same call wrote"""
    g = wc.load_case(name)
    w = U.Waterfall(g["channels"], wc.config_of(g))
    if name == "wrap":
        assert step > 2 * w.plan.wfall_size
    if (name, step) == ("step5", 2):
        assert not g["drawn"][0, :4].any()
    if (name, step) == ("step5", 13):
        assert g["drawn"][0, :13].sum() == 2
    run_calls(g, w, step)
    st = w.state()
    assert st["wfall_line"] % w.plan.wfall_size == int(g["counters"][0]) % w.plan.wfall_size and st["wfall_line_update"] == int(g["counters"][1])


def tiled(C):
    """C channels of 128 x 9 at magnify 2: channel c has the lines and frequencies of channel (c // 6) % 3 of the case
    shift_m(c % 6), so neighbouring channels differ in every line and every offset_pixel"""
    parts = [wc.load_case(f"shift_m{m}") for m in range(6)]
    F = parts[0]["frames"]
    assert all(p["frames"] == F and p["W"] == 128 and p["channels"] == 3 for p in parts)
    lines = np.stack([parts[c % 6]["lines"][(c // 6) % 3] for c in range(C)])
    hz = np.stack([parts[c % 6]["center_hz"][(c // 6) % 3] for c in range(C)])
    return parts[2]["cfg"], lines, hz


def test_130_channels_against_the_host_twin(cuda):
    C = 130
    cfg, lines, hz = tiled(C)
    dev, host = U.Waterfall(C, U.wfall_config(**cfg)), U.Waterfall(C, U.wfall_config(**cfg), host=True)
    out = device_outputs(dev, 0)
    want = np.full(out["image"].shape, wc.SENTINEL, np.uint16)
    offsets = set()
    for first in range(0, lines.shape[1], 7):
        part, part_hz = np.ascontiguousarray(lines[:, first:first + 7]), np.ascontiguousarray(hz[:, first:first + 7])
        drawn = device_outputs(dev, part.shape[1])["drawn"]
        dev.process_lines(put(part), put(part_hz, np.int32), image=out["image"], drawn=drawn)
        got_host = host.process_lines_host(part, part_hz, want)
        got = image_of(out["image"])
        assert (drawn.cpu().numpy() == got_host["drawn"]).all()
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (first, len(bad), tuple(bad[0]))
        offsets |= {int((want[c, -1] == 0).sum()) for c in range(C)}
    assert len(offsets) > 8          # rows of many different paddings were among those compared
    assert dev.state() == host.state()


@pytest.mark.parametrize("width,height", [(128, 5), (200, 9), (480, 70), (511, 3), (511, 85)])
def test_widths_against_the_host_twin(cuda, width, height):
    """511 is no multiple of 8: with three rows the second channel's image starts off a 16-byte boundary and rows end
    inside a 16-byte piece; 480 x 70 is the panel; shifts of a few pixels in both directions and beyond the width"""
    rng = np.random.default_rng(width * 1000 + height)
    C, F = 3, 9
    cfg = U.wfall_config(width=width, height=height, color_scheme=2, vert_step_size=1, magnify=1, dmod_mode=U.DEMOD_DIGI,
                         digital_mode=U.DIGITAL_MODE_RTTY, marker_colour=0xF81F)
    lines = rng.integers(0, 66, (C, F, width), dtype=np.uint8)
    hz = (7000000 + rng.choice([0, 0, 40, -40, 900, -2500, 60000, -60000], (C, F))).astype(np.uint32)
    dev, host = U.Waterfall(C, cfg), U.Waterfall(C, cfg, host=True)
    for first, n in ((0, 4), (4, 1), (5, 4)):
        out = device_outputs(dev, n)
        dev.process_lines(put(lines[:, first:first + n]), put(hz[:, first:first + n], np.int32), **out)
        want = host.process_lines_host(np.ascontiguousarray(lines[:, first:first + n]), np.ascontiguousarray(hz[:, first:first + n]))
        got = image_of(out["image"])
        bad = np.argwhere(got != want["image"])
        assert len(bad) == 0, (first, len(bad), tuple(bad[0]))
        assert (out["drawn"].cpu().numpy() == want["drawn"]).all()


def test_an_image_off_the_16_byte_grid(cuda):
    """the image at every 2-byte offset inside a larger tensor: the pixels before and behind the whole 16-byte pieces,
    and nothing written outside the image"""
    import torch
    g = wc.load_case("w200_h9")
    C, H, W = g["channels"], g["H"], g["W"]
    want = wc.expected_image(g, g["frames"] - 1)
    for lead in range(8):
        w = U.Waterfall(C, wc.config_of(g))
        flat = torch.full((lead + C * H * W + 24,), IMAGE_SENTINEL, dtype=torch.int16, device="cuda")
        image = flat[lead:lead + C * H * W].view(C, H, W)
        w.process_lines(put(g["lines"]), put(g["center_hz"], np.int32), image=image)
        w.synchronize()
        got = image_of(flat)
        assert (got[lead:lead + C * H * W].reshape(C, H, W) == want).all(), lead
        assert (got[:lead] == wc.SENTINEL).all() and (got[lead + C * H * W:] == wc.SENTINEL).all(), lead


def test_optional_outputs_and_sentinels(cuda):
    g = wc.load_case("step2")
    lines, hz, F = put(g["lines"]), put(g["center_hz"], np.int32), g["frames"]
    want = wc.expected_image(g, F - 1)
    # image only
    w = U.Waterfall(g["channels"], wc.config_of(g))
    out = device_outputs(w, F)
    w.process_lines(lines, hz, image=out["image"])
    assert (image_of(out["image"]) == want).all() and bool((out["drawn"] == DRAWN_SENTINEL).all())
    # drawn only
    w = U.Waterfall(g["channels"], wc.config_of(g))
    out = device_outputs(w, F)
    w.process_lines(lines, hz, drawn=out["drawn"])
    assert (out["drawn"].cpu().numpy() == g["drawn"]).all() and bool((out["image"] == IMAGE_SENTINEL).all())
    # neither, through a null io: ring and counters move all the same
    w = U.Waterfall(g["channels"], wc.config_of(g))
    head = lines[:, :F - 2].contiguous()
    w._call("process_lines", w._ptr(head), None, F - 2, None)
    out = device_outputs(w, 2)
    assert g["drawn"][0, F - 2] == 1 and (g["center_hz"] == 0).all()
    w.process_lines(lines[:, F - 2:].contiguous(), hz[:, F - 2:].contiguous(), **out)
    assert (image_of(out["image"]) == want).all() and (out["drawn"].cpu().numpy() == g["drawn"][:, F - 2:]).all()
    # a call in which no frame draws leaves the image alone
    w = U.Waterfall(g["channels"], wc.config_of(g))
    out = device_outputs(w, 1)
    assert g["drawn"][0, 0] == 0
    w.process_lines(lines[:, :1].contiguous(), hz[:, :1].contiguous(), **out)
    assert bool((out["image"] == IMAGE_SENTINEL).all()) and (out["drawn"].cpu().numpy() == 0).all()


def test_reset_and_null_center(cuda):
    g = wc.load_case("w200_h9")
    w = U.Waterfall(g["channels"], wc.config_of(g))
    w.process_lines(put(g["lines"][:, :3]))
    assert w.state()["double_line_start"] == 1
    w.reset()
    assert w.state() == dict(wfall_line=0, double_line_start=0, wfall_line_update=0)
    run_calls(g, w, 2)
    g = wc.load_case("pal3")
    assert (g["center_hz"] == 0).all()
    run_calls(g, U.Waterfall(g["channels"], wc.config_of(g)), 4, center=False)
    # frequencies given in one call and null in the next: the null frames stand at 0
    g = wc.load_case("far_above")
    dev, host = U.Waterfall(g["channels"], wc.config_of(g)), U.Waterfall(g["channels"], wc.config_of(g), host=True)
    out = device_outputs(dev, 0)
    dev.process_lines(put(g["lines"][:, :5]), put(g["center_hz"][:, :5], np.int32))
    dev.process_lines(put(g["lines"][:, 5:]), None, image=out["image"])
    host.process_lines_host(np.ascontiguousarray(g["lines"][:, :5]), np.ascontiguousarray(g["center_hz"][:, :5]))
    want = host.process_lines_host(np.ascontiguousarray(g["lines"][:, 5:]))["image"]
    assert (image_of(out["image"]) == want).all()


def test_refusals_on_the_device(cuda):
    import ctypes as C
    import torch
    lib = U.load()
    w = U.Waterfall(2, U.wfall_config(width=128, height=4))
    buf = torch.zeros(2 * 8 * 128 + 2 * 4 * 128 * 2, dtype=torch.uint8, device="cuda")
    io = U.WfallIo(image=buf.data_ptr() + 2 * 8 * 128 - 2)
    assert lib.uhsdr_wfall_process_lines(w.handle, C.c_void_p(buf.data_ptr()), None, 8, C.byref(io)) == U.UHSDR_ARGUMENT_ERROR
    io = U.WfallIo(image=buf.data_ptr() + 2 * 8 * 128 + 1)
    assert lib.uhsdr_wfall_process_lines(w.handle, C.c_void_p(buf.data_ptr()), None, 8, C.byref(io)) == U.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_wfall_process_lines_host(w.handle, C.c_void_p(buf.data_ptr()), None, 8, None) == U.UHSDR_ARGUMENT_ERROR
    assert w.state() == dict(wfall_line=0, double_line_start=0, wfall_line_update=0)


def test_chained_behind_the_display_stage_on_one_stream(cuda):
    """frames of FFT_AVGData through Display.process_avg, its wfall row straight into Waterfall.process_lines on a
    stream of their own, no copy and no synchronise between them: the bytes and the images the firmware formed from
    the same averages behind a harness spectrum run"""
    import torch
    g = wc.load_case(wc.SPEC_CASE)
    with np.load(os.path.join(wc.GOLDEN, f"spec_{str(g['spec'])}.npz")) as z:
        avg = np.ascontiguousarray(z["avg"][:g["channels"]])
    C, F = g["channels"], g["frames"]
    assert avg.shape[:2] == (C, F)
    stream = torch.cuda.Stream()
    d = U.Display(C, U.display_config(**json.loads(str(g["display"]))), stream=stream.cuda_stream)
    w = U.Waterfall(C, wc.config_of(g), stream=stream.cuda_stream)
    image = device_outputs(w, 0)["image"]
    assert F % 4 == 0 and (g["center_hz"] == 0).all()
    parts = [put(avg[:, first:first + 4]) for first in range(0, F, 4)]
    rows = [torch.full((C, 4, g["W"]), 0xEE, dtype=torch.uint8, device="cuda") for _ in parts]
    torch.cuda.synchronize()            # the inputs were made on the default stream
    for first, part, bytes_row in zip(range(0, F, 4), parts, rows):
        d.process_avg(part, wfall=bytes_row)
        w.process_lines(bytes_row, image=image)
        w.synchronize()
        assert (bytes_row.cpu().numpy() == g["lines"][:, first:first + 4]).all(), first
        wc.check_image(g, image_of(image), first + 3, "behind the display stage")
