"""The waterfall-image fixtures (tests/golden/wfall_*.npz, recorded from the reference firmware by
tools/wfall/make_wfall_golden.py): the configuration, the byte lines and centre frequencies per
channel and frame, `drawn`, the image of every frame that drew in the order of the firmware's
UiLcdHy28_BulkPixel_PutBuffer calls, the ring line each frame wrote, and what the firmware computed
for the plan (wfall_size, repeat, marker_num, hz_per_pixel, rx_carrier_pos, marker_pos, the 65
colours) with its counters after the last frame.  Loaded once and shared; nothing here is modified by
a test.  What the set as a whole must show is asserted by check_set()."""
import functools
import glob
import json
import os

import numpy as np

from uhsdr_amd import wfall

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("wfall_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "wfall_*.npz"))
               if not p.endswith("wfall_tables.npz"))
SPEC_CASE = "spec_p48_usb_256"        # behind a harness spectrum run: its lines are the display stage's
SENTINEL = 0xA5A5                     # no palette has it, nor is it the cases' marker colour


@functools.lru_cache(maxsize=None)
def palettes():
    with np.load(os.path.join(GOLDEN, "wfall_tables.npz")) as z:
        return z["palettes"]


def config_of(g, **over):
    return wfall.wfall_config(**dict(g["cfg"], **over))


@functools.lru_cache(maxsize=None)
def load_case(name):
    with np.load(os.path.join(GOLDEN, f"wfall_{name}.npz")) as z:
        g = {k: z[k] for k in z.files}
    g["name"] = name
    g["cfg"] = json.loads(str(g.pop("config")))
    C, F, W = g["lines"].shape
    H = g["cfg"]["height"]
    g["channels"], g["frames"], g["W"], g["H"] = C, F, W, H
    assert 1 <= C <= 3 and W == g["cfg"]["width"], name
    assert g["lines"].dtype == np.uint8 and g["center_hz"].dtype == np.uint32 and g["center_hz"].shape == (C, F), name
    assert g["image"].dtype == np.uint16 and g["image"].shape == (C, F, H, W) and g["drawn"].shape == (C, F), name
    assert (g["drawn"] == g["drawn"][0]).all(), name            # the counters never look at the data
    assert not (g["image"] == SENTINEL).any() and g["cfg"]["marker_colour"] != SENTINEL, name
    return g


def expected_image(g, frame):
    """the panel after frames 0 .. frame: the image of the last one of them that drew, [C][H][W]; None: none drew yet"""
    drew = np.flatnonzero(g["drawn"][0, :frame + 1])
    return g["image"][:, drew[-1]] if len(drew) else None


def check_image(g, got, frame, what=""):
    want = expected_image(g, frame)
    if want is None:
        assert (np.asarray(got) == SENTINEL).all(), f"{g['name']} {what}: written though no frame up to {frame} drew"
        return
    bad = np.argwhere(np.asarray(got) != want)
    assert len(bad) == 0, (f"{g['name']} {what}: image after frame {frame} differs at {len(bad)} of {want.size} pixels, first "
                           f"(channel, row, column) {tuple(bad[0])}: got {np.asarray(got)[tuple(bad[0])]:#06x} want {want[tuple(bad[0])]:#06x}")


def check_set():
    """every palette entry reached; left and right padding; the width - 1 quirk from both signs; a frame that draws
    nothing; both values of doubleLineStart on the first row; two markers for RTTY, none on screen when pushed off;
    the panel's 35 lines put three times; the memory-limited ring; an odd height inside a repeat"""
    reached = {k: set() for k in range(5)}
    left = right = idle = 0
    for name in CASES:
        g = load_case(name)
        drawn = g["drawn"].astype(bool)
        reached[g["cfg"]["color_scheme"]] |= set(g["image"][drawn].ravel().tolist())
        idle += int((~drawn).sum())
        rows = g["image"][drawn].reshape(-1, g["W"])
        body = (rows != 0) & (rows != g["cfg"]["marker_colour"])
        left += int((~body[:, 0] & body[:, -1]).sum())
        right += int((body[:, 0] & ~body[:, -1]).sum())
        if name in ("far_below", "far_above"):
            assert int((~body[:, :-1].any(axis=1) & body[:, -1]).sum()) > 0 and int((body[:, 0] & ~body[:, -1]).sum()) == 0, name
    for k in range(5):
        assert set(palettes()[k].tolist()) <= reached[k], k
    assert left > 0 and right > 0 and idle > 0

    def head_run(image):
        n = 1
        while n < len(image) and (image[n] == image[0]).all():
            n += 1
        return n
    g = load_case("w200_h9")
    assert {head_run(g["image"][c, f]) for c in range(g["channels"]) for f in range(g["frames"]) if g["drawn"][c, f]} == {1, 2}
    assert tuple(load_case("panel")["plan_ints"][:2]) == (35, 2)
    g = load_case("memlimit")
    assert g["plan_ints"][0] == 20480 // g["W"] < g["H"] // 2
    g = load_case("repeat2_odd")
    assert tuple(g["plan_ints"][:2]) == (g["H"] // 2, 2) and g["H"] % 2 == 1
    g = load_case("wrap")
    assert g["frames"] > 2 * g["plan_ints"][0]

    def on_screen(name):
        g = load_case(name)
        return int(g["plan_ints"][2]), int((g["image"][0, np.flatnonzero(g["drawn"][0])[0], 0] == g["cfg"]["marker_colour"]).sum())
    assert on_screen("mk_rtty") == (2, 2) and on_screen("mk_bpsk") == (2, 2)
    assert on_screen("mk_off_right") == (1, 0) and on_screen("mk_negative") == (1, 0)
    assert on_screen("mk_negative_low_bits") == (1, 1) and load_case("mk_negative_low_bits")["plan_floats"][2] < -65000
    g = load_case("above")
    assert (g["lines"] == 64).any() and (g["lines"] == 255).any()
    assert {load_case(f"shift_m{m}")["cfg"]["magnify"] for m in range(6)} == set(range(6))
