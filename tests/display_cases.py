"""The display-stage fixtures (tests/golden/display_*.npz, recorded from the reference firmware by
tools/display/make_display_golden.py): the configuration, the frames of FFT_AVGData (taken from the
spectrum recording the case names, or stored), checked against the recorded crc32, `edge` per channel
and frame, the four outputs per channel and frame, sd.db_scale / agc_rate / wfall_contrast as the
firmware computed them and whether the last column reads the edge.  Loaded once and shared; nothing
here is modified by a test.  What the set as a whole must show is asserted by check_set()."""
import functools
import glob
import json
import os
import zlib

import numpy as np

from uhsdr_amd import display

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("display_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "display_*.npz"))
               if not p.endswith("display_tables.npz"))
SPEC_CASES = [n for n in CASES if n.startswith("p48_")]       # frames of a spec_*.npz recording
NYQUIST = "iq_nyquist_512"                                     # its own I/Q, with an edge that shows
OUTPUTS = [name for name, _ in display.OUTPUTS]
NEGATIVE = "edge_m1e6"      # a negative last column: its conversion is the library's definition


def same(a, b):
    """bit for bit, two NaNs equal"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float32:
        return a == b
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def config_of(g, **over):
    return display.display_config(**dict(g["cfg"], **over))


@functools.lru_cache(maxsize=None)
def load_case(name):
    with np.load(os.path.join(GOLDEN, f"display_{name}.npz")) as z:
        g = {k: z[k] for k in z.files}
    g["name"] = name
    g["cfg"] = json.loads(str(g.pop("config")))
    source = json.loads(str(g.pop("source")))
    g["spec"] = source.get("spec")
    if g["spec"]:
        with np.load(os.path.join(GOLDEN, f"spec_{g['spec']}.npz")) as z:
            g["avg"], g["iq"], g["spec_args"] = z["avg"], z["iq"], json.loads(str(z["args"]))
    elif source.get("iq"):
        g["spec_args"] = source["args"]
    assert zlib.crc32(g["avg"].tobytes()) == int(g["crc32"]), name
    C, F, L = g["avg"].shape
    g["channels"], g["frames"], g["L"] = C, F, L
    g["W"] = g["scope"].shape[2]
    assert L == g["cfg"]["fft_len"] and 2 <= C <= 4 and F <= 24, name
    for out, dt in display.OUTPUTS:
        assert g[out].dtype == dt and g[out].shape == ((C, F, g["W"]) if out in display.WIDE else (C, F)), (name, out)
    assert g["edge"].shape == (C, F) and g["edge"].dtype == np.float32 and g["plan"].shape == (3,), name
    return g


def check_set():
    """more than 20 heights, 63 reached and not exceeded, the clipped case at its limit, the offset moving both ways,
    the edge read at 480 and not at 256 -> 200"""
    heights, colours = set(), set()
    for name in CASES:
        g = load_case(name)
        if name == NEGATIVE:
            continue
        heights |= set(g["scope"].ravel().tolist())
        colours |= set(g["wfall"].ravel().tolist())
    assert len(heights) > 20 and max(colours) == 63, (sorted(heights), sorted(colours))
    clip = load_case("scopeh16")
    assert clip["scope"].max() == 15 and (clip["scope"] == 15).sum() > 10
    step = load_case("step")
    d = np.diff(step["offset"], axis=1)
    assert (d > 0).any() and (d < 0).any() and step["frames"] >= 20
    assert load_case("p48_usb_512")["reads_edge"] == 1 and load_case("step")["reads_edge"] == 1 and load_case("w256_200")["reads_edge"] == 0
    nan = load_case("allnan")
    assert (nan["min"][0] == 100000).all() and (nan["wfall"][0] == 0).all()
    zero = load_case("scale0")
    assert (zero["min"][:, 1:] == zero["offset"][:, :-1]).all()        # factor 0: every sig is the offset


def check_rows(g, rows, first=0, frames=None, what=""):
    """rows: the four outputs by name, computed for the frames from `first` on"""
    n = frames if frames is not None else np.shape(rows[OUTPUTS[0]])[1]
    for out in OUTPUTS:
        got = np.ascontiguousarray(rows[out])[:, :n]
        want = g[out][:, first:first + n]
        bad = np.argwhere(~same(got, want))
        assert len(bad) == 0, (f"{g['name']} {what}: {out} differs at {len(bad)} of {got.size} places, first "
                               f"{tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}")
