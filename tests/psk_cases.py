"""The BPSK fixtures (tests/golden/psk_*.npz, recorded from the reference firmware by
tools/psk/make_psk_golden.py) with their inputs regenerated from uhsdr_amd.synth and checked
against the recorded crc32, and with what each recording must show asserted on load.  Loaded once
and shared; nothing here is modified by a test.
CASES: the decoder alone (12 ksps audio); CHAIN_CASES: through the receive chain (I/Q)."""
import functools
import glob
import os

from uhsdr_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_names = sorted(os.path.basename(p)[len("psk_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "psk_*.npz")))
CASES = [n for n in _names if not n.startswith("chain_")]
CHAIN_CASES = [n for n in _names if n.startswith("chain_")]

# what the recorded bytes of a case must show: (expect, least number of bytes), fixed here and not
# read from the file
EXPECT = {
    "clean31": ("sent", 0), "clean63": ("sent", 0), "clean125": ("sent", 0), "chartable125": ("sent", 256),
    "noisy_a": ("count", 20), "noisy_b": ("garbled", 20),
    "df0p5": ("garbled", 0), "df1": ("garbled", 0), "df2": ("garbled", 0),
    "tiny": ("count", 30), "floor": ("nothing", 0), "huge": ("sent", 0), "overflow": ("nothing", 0),
    "idle60": ("recorded", 0), "burst": ("twice", 0), "silence": ("nothing", 0), "midchar": ("recorded", 0),
    **{f"offsets63_{k}": ("sent", 0) for k in range(8)},
}


@functools.lru_cache(maxsize=None)
def load_case(name):
    g = synth.psk_fixture(os.path.join(GOLDEN, f"psk_{name}.npz"))
    expect, least = EXPECT[name]
    printed, sent = bytes(g["chars"]), g["sent"]
    assert len(printed) >= least, name
    if expect == "sent":
        assert sent in printed, name
    elif expect == "twice":
        assert printed.count(sent) == 2, name
    elif expect == "garbled":
        assert sent not in printed, name
    elif expect == "nothing":
        assert len(printed) == 0, name
    g["name"] = name
    return g


@functools.lru_cache(maxsize=None)
def load_chain_case(name):
    g = synth.psk_chain_fixture(os.path.join(GOLDEN, f"psk_{name}.npz"))
    assert str(g["message"]).encode() in bytes(g["chars"]), name
    return g
