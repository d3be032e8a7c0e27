"""The RTTY fixtures (tests/golden/rtty_*.npz, recorded from the reference firmware by
tools/rtty/make_rtty_golden.py) with their inputs regenerated from uhsdr_amd.synth and checked
against the recorded crc32.  Loaded once and shared; nothing here is modified by a test.
CASES: the decoder alone (12 ksps audio); CHAIN_CASES: through the receive chain (I/Q)."""
import functools
import glob
import os

from uhsdr_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_names = sorted(os.path.basename(p)[len("rtty_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "rtty_*.npz")))
CASES = [n for n in _names if not n.startswith("chain_")]
CHAIN_CASES = [n for n in _names if n.startswith("chain_")]


@functools.lru_cache(maxsize=None)
def load_case(name):
    return synth.rtty_fixture(os.path.join(GOLDEN, f"rtty_{name}.npz"))


@functools.lru_cache(maxsize=None)
def load_chain_case(name):
    return synth.rtty_chain_fixture(os.path.join(GOLDEN, f"rtty_{name}.npz"))
