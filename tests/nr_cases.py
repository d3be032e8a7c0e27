"""The noise-reduction fixtures (tests/golden/nr_*.npz, recorded from the reference firmware by
tools/nr/make_nr_golden.py) with their inputs regenerated from uhsdr_amd.synth.nr_audio and checked
against the recorded crc32, and with what each recording must show asserted on load.  Loaded once
and shared; nothing here is modified by a test.
CASES: the frame stage alone; STREAM_CASES: the 12 ksps stream around it."""
import functools
import glob
import os
import zlib

import numpy as np

from uhsdr_amd import nr, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_names = sorted(os.path.basename(p)[len("nr_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "nr_*.npz")))
STREAM_CASES = [n[len("stream_"):] for n in _names if n.startswith("stream_")]
CASES = [n for n in _names if not n.startswith("stream_") and n not in ("tables", "icfft")]
FRAME = nr.FRAME

# what a recording must show, fixed here and not read from the file: the NN values it has to
# contain, and the band (VAD_low, VAD_high) the library derives for its configuration
SHOW = {
    "ssb6k_snr10": ((), (12, 128)), "ssb6k_snrm3_weak": ((), (12, 128)), "ssb6k_snr20_strong": ((), (12, 128)),
    "ssb6k_snr3_asnr15": ((), (12, 128)), "cw6k_snr5": ((), (12, 21)), "wide12k_snr10": ((), (2, 64)),
    "wide12k_snrm3": ((), (2, 78)), "equal_band": ((), (21, 22)), "wrap126": ((1,), (126, 100)),
    "restart": ((), (12, 128)), "nn_all": ((1, 3, 5, 7, 9), (12, 128)), "width5_thr100": ((11,), (12, 128)),
}


def config_of(g):
    return nr.nr_config(**g["cfg"])


@functools.lru_cache(maxsize=None)
def load_case(name):
    g = synth.nr_fixture(os.path.join(GOLDEN, f"nr_{name}.npz"))
    g["name"] = name
    g["frames"] = len(g["audio"]) // FRAME
    assert len(g["nn"]) == g["frames"] >= 41, name
    ft = g["first_time"]
    assert ft[18] == 2 and ft[19] == 3, name                  # the 20-frame start-up
    g["running"] = ft == 3
    reset = int(g["reset"])
    if reset >= 0:
        assert ft[reset - 1] == 3 and ft[reset] == 2 and ft[reset + 19] == 3, name
        g["running"][:reset + 19] &= np.arange(reset + 19) < reset       # NN is stale while the restart averages
    g["running"][:19] = False
    nn_seen, band = SHOW[name]
    assert set(nn_seen) <= set(g["nn"][g["running"]].tolist()), name
    assert nr.nr_band(config_of(g)) == band, name
    if name == "wrap126":
        assert np.isnan(g["power_ratio"][g["running"]]).all(), name
    else:
        assert np.isfinite(g["power_ratio"][g["running"]]).all(), name
    if "out" in g:
        g["out_crc"] = np.array([zlib.crc32(f.tobytes()) for f in g["out"]], dtype=np.uint32)
    return g


def check_frames(g, y, first=0, what=""):
    """y: float32 [frames][128] computed for the frames from `first` on, against the recording"""
    y = np.ascontiguousarray(y).reshape(-1, FRAME)
    n = len(y)
    if "out" in g:
        bad = np.flatnonzero((y.view(np.uint32) != g["out"][first:first + n].view(np.uint32)).any(axis=1))
    else:
        crc = np.array([zlib.crc32(f.tobytes()) for f in y], dtype=np.uint32)
        bad = np.flatnonzero(crc != g["out_crc"][first:first + n])
    assert len(bad) == 0, (g["name"], what, "first differing frame", first + int(bad[0]), "of", len(bad))


@functools.lru_cache(maxsize=None)
def load_stream_case(name):
    g = synth.nr_fixture(os.path.join(GOLDEN, f"nr_stream_{name}.npz"))
    g["name"] = name
    out = g["out"]
    assert len(out) == len(g["audio"]) and len(out) % 8 == 0, name
    decimated = g["cfg"]["width_hz"] < 2701
    # the FIFO's latency as the recording shows it: silence for two frames at the frames' rate
    quiet = 512 if decimated else 256
    assert not out[:quiet].any() and out[quiet:quiet + 32].any(), name
    return g
