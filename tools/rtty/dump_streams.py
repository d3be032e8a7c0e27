#!/usr/bin/env python3
"""The RTTY fixtures' inputs and expected bytes as one binary file for tools/rtty/rtty_sanitize.c:
int32 cases; per case int32 shift_idx, speed_idx, stopbits_idx, atc_disable, samples, nchars, then
the float32 samples and the expected characters.

    python3 tools/rtty/dump_streams.py /tmp/rtty_streams.bin"""
import glob
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from uhsdr_amd import synth  # noqa: E402

FILES = sorted(f for f in glob.glob(os.path.join(ROOT, "tests", "golden", "rtty_*.npz")) if "rtty_chain_" not in f)

with open(sys.argv[1], "wb") as f:
    f.write(struct.pack("<i", len(FILES)))
    for name in FILES:
        g = synth.rtty_fixture(name)
        f.write(struct.pack("<6i", *g["config"], len(g["audio"]), len(g["chars"])))
        f.write(g["audio"].tobytes())
        f.write(g["chars"].tobytes())
