#!/usr/bin/env python3
"""Write the display-stage fixtures with their frames and plans into one binary file for
tools/display/display_sanitize.c:

  python3 tools/display/dump_cases.py /tmp/display_cases.bin

File: int32 count, then per case int32 sizeof(uhsdr_display_plan), channels, frames, fft_len, width,
the plan (uhsdr_display_plan_build of the case's configuration), float32 avg[channels][frames][fft_len],
float32 edge[channels][frames], and the recorded rows: uint16 scope[channels][frames][width], uint8
wfall[channels][frames][width], float32 offset[channels][frames], float32 min[channels][frames]."""
import ctypes as C
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import display_cases  # noqa: E402
from uhsdr_amd import display  # noqa: E402


def main():
    out = []
    for name in display_cases.CASES:
        g = display_cases.load_case(name)
        plan = display.display_plan(display_cases.config_of(g))
        rows = b"".join(np.ascontiguousarray(g[k]).tobytes() for k in display_cases.OUTPUTS)
        out.append(struct.pack("<5i", C.sizeof(plan), g["channels"], g["frames"], g["L"], g["W"]) + bytes(plan)
                   + np.ascontiguousarray(g["avg"]).tobytes() + np.ascontiguousarray(g["edge"]).tobytes() + rows)
    with open(sys.argv[1], "wb") as f:
        f.write(struct.pack("<i", len(out)) + b"".join(out))
    print(f"{len(out)} cases")


if __name__ == "__main__":
    main()
