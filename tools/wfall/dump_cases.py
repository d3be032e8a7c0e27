#!/usr/bin/env python3
"""Write the waterfall-image fixtures with their plans into one binary file for
tools/wfall/wfall_sanitize.c:

  python3 tools/wfall/dump_cases.py /tmp/wfall_cases.bin

File: int32 count, then per case int32 sizeof(uhsdr_wfall_plan), channels, frames, width, height, the
plan (uhsdr_wfall_plan_build of the case's configuration), uint8 lines[channels][frames][width], uint32
center_hz[channels][frames], uint8 drawn[channels][frames], and uint16 image[channels][frames][height][width]
as recorded (zeros where the frame did not draw)."""
import ctypes as C
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wfall_cases  # noqa: E402
from uhsdr_amd import wfall  # noqa: E402


def main():
    out = []
    for name in wfall_cases.CASES:
        g = wfall_cases.load_case(name)
        plan = wfall.wfall_plan(wfall_cases.config_of(g))
        out.append(struct.pack("<5i", C.sizeof(plan), g["channels"], g["frames"], g["W"], g["H"]) + bytes(plan)
                   + b"".join(np.ascontiguousarray(g[k]).tobytes() for k in ("lines", "center_hz", "drawn", "image")))
    with open(sys.argv[1], "wb") as f:
        f.write(struct.pack("<i", len(out)) + b"".join(out))
    print(f"{len(out)} cases")


if __name__ == "__main__":
    main()
