#!/usr/bin/env python3
"""The BPSK fixtures' inputs and expected bytes as one binary file for tools/psk/psk_sanitize.c:
int32 cases; per case int32 speed_idx, samples, nchars, then the float32 samples and the expected
characters.

    python3 tools/psk/dump_streams.py /tmp/psk_streams.bin"""
import glob
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from uhsdr_amd import synth  # noqa: E402

FILES = sorted(f for f in glob.glob(os.path.join(ROOT, "tests", "golden", "psk_*.npz")) if "psk_chain_" not in f)

with open(sys.argv[1], "wb") as f:
    f.write(struct.pack("<i", len(FILES)))
    for name in FILES:
        g = synth.psk_fixture(name)
        f.write(struct.pack("<3i", g["speed"], len(g["audio"]), len(g["chars"])))
        f.write(g["audio"].tobytes())
        f.write(g["chars"].tobytes())
