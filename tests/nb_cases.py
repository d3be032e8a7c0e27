"""The noise-blanker fixtures (tests/golden/nb_*.npz, recorded from the reference firmware by
tools/nb/make_nb_golden.py) with their inputs regenerated from uhsdr_amd.synth.nb_audio and checked
against the recorded crc32, and with what each recording must show asserted on load.  Loaded once
and shared; nothing here is modified by a test.
CASES: the blanker's frames alone; STREAM_CASES: the 12 ksps stream with the blanker in it."""
import functools
import glob
import os

import numpy as np

from uhsdr_amd import nb, nr, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_names = sorted(os.path.basename(p)[len("nb_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "nb_*.npz")))
STREAM_CASES = [n[len("stream_"):] for n in _names if n.startswith("stream_")]
CASES = [n for n in _names if not n.startswith("stream_")]
FRAME, DELAY = nb.FRAME, nb.DELAY

# what a recording must show, fixed here and not read from the file: the setting, and
#   "changed"  some samples differ from the input delayed by 13
#   "burst"    some frame has more than 28 changed samples: five repairs
#   "walk"     repairs start in the last quarter of a frame and in the first quarter of one
#   "every"    every frame after the first is changed
#   "same"     the output is exactly the delayed input
#   "finite"   changed, and every sample finite
#   "nan"      exactly one NaN in the output, and the frames that see the NaN or the infinity unchanged
SHOW = {
    "sparse_s1": (1, "changed"), "sparse_s8": (8, "changed"), "sparse_s15": (15, "changed"), "burst8": (8, "burst"),
    "walk": (8, "walk"), "tone": (8, "changed"), "noise_s15": (15, "every"), "clean_s8": (8, "same"), "dc": (8, "same"),
    "silence": (8, "same"), "tiny": (8, "same"), "big": (8, "finite"), "nan_inf": (8, "nan"),
}
# the stream cases: nb_setting, nr_bypass, filter width
STREAM_SHOW = {"nb_wide": (8, 1, 3200), "nb_narrow": (8, 1, 2400), "nb_nr_2700": (8, 0, 2700), "nb_nr_wide": (8, 0, 3200)}


def same(a, b):
    """bit for bit, two NaNs equal"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def changed(x, y, delay=DELAY):
    """which output samples differ from the input `delay` samples earlier"""
    d = np.concatenate([np.zeros(delay, np.float32), x])[:len(y)]
    return ~same(d, y)


def run_starts(mask):
    m = np.concatenate([[False], mask])
    return np.flatnonzero(m[1:] & ~m[:-1])


def config_of(g):
    return nb.nb_config(**g["cfg"])


@functools.lru_cache(maxsize=None)
def load_case(name):
    g = synth.nb_fixture(os.path.join(GOLDEN, f"nb_{name}.npz"))
    g["name"] = name
    x, y = g["audio"], g["out"]
    g["frames"] = len(x) // FRAME
    assert 48 <= g["frames"] <= 60 and len(y) == len(x), name
    setting, show = SHOW[name]
    assert g["cfg"] == {"nb_setting": setting}, name
    ch = changed(x, y)
    g["changed"] = ch
    per_frame = ch.reshape(-1, FRAME).sum(axis=1)
    assert ch.any() == (show != "same"), name
    if show == "burst":
        assert per_frame.max() > 28, name
    if show == "walk":
        at = (run_starts(ch) - DELAY) % FRAME
        assert (at >= 96).any() and (at < 32).any(), name
    if show == "every":
        assert (per_frame[1:] > 0).all(), name
    if show == "nan":
        assert int(np.isnan(y).sum()) == 1 and int(np.isnan(x).sum()) == 1 and int(np.isinf(x).sum()) == 1, name
        for at in np.flatnonzero(~np.isfinite(x)):
            # the frames whose analysis sees the sample: it lies in wb[13 .. 141) of the frame it arrives in or the next
            f = at // FRAME
            assert not ch[f * FRAME:(f + 2) * FRAME].any(), (name, at)
    else:
        assert np.isfinite(y).all(), name
    return g


def check_sparse_grows():
    """the same input at settings 1, 8 and 15: a higher setting changes more samples"""
    c = [int(load_case(n)["changed"].sum()) for n in ("sparse_s1", "sparse_s8", "sparse_s15")]
    assert 0 < c[0] < c[1] < c[2], c
    assert np.array_equal(load_case("sparse_s1")["audio"], load_case("sparse_s15")["audio"])


def check_frames(g, y, first=0, what=""):
    """y: float32 computed for the frames from `first` on, against the recording"""
    y = np.ascontiguousarray(y).reshape(-1)
    want = g["out"][first * FRAME:first * FRAME + len(y)]
    bad = np.flatnonzero(~same(y, want))
    assert len(bad) == 0, (g["name"], what, "first differing sample", first * FRAME + int(bad[0]), "of", len(bad))


def stream_config_of(g):
    return nr.nr_config(**g["cfg"])


@functools.lru_cache(maxsize=None)
def load_stream_case(name):
    g = synth.nb_fixture(os.path.join(GOLDEN, f"nb_stream_{name}.npz"))
    g["name"] = name
    x, out = g["audio"], g["out"]
    assert len(out) == len(x) == 600 * 8, name
    setting, bypass, width = STREAM_SHOW[name]
    assert (g["cfg"]["nb_setting"], g["cfg"]["nr_bypass"], g["cfg"]["width_hz"]) == (setting, bypass, width), name
    quiet = 512 if width < 2701 else 256
    assert not out[:quiet].any() and out[quiet:quiet + 64].any() and np.isfinite(out).all(), name
    if name == "nb_wide":
        # the blanker alone at 12 ksps: silence for two frames and the blanker's 13 samples, then the input apart from the repairs
        ch = changed(x, out, 256 + DELAY)
        assert not out[:256 + DELAY].any() and 0 < ch.sum() <= 7 * 5 * (len(x) // FRAME), name
        g["changed"] = ch
    return g
