#!/usr/bin/env python3
"""Write the signal-meter fixtures with their frames and plans into one binary file for
tools/meter/meter_sanitize.c:

  python3 tools/meter/dump_cases.py /tmp/meter_cases.bin

File: int32 count, then per case int32 sizeof(uhsdr_meter_plan), channels, frames, fft_len, the plan
(uhsdr_meter_plan_build of the case's configuration), float32 mag[channels][frames][fft_len], uint8
cw_signal[channels][frames], and the six recorded rows [channels][frames] of four bytes each in the
order of uhsdr_meter_io."""
import ctypes as C
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import meter_cases  # noqa: E402
from uhsdr_amd import meter  # noqa: E402


def main():
    out = []
    for name in meter_cases.CASES:
        g = meter_cases.load_case(name)
        plan = meter.meter_plan(meter_cases.config_of(g))
        rows = b"".join(np.ascontiguousarray(g[k]).tobytes() for k in meter_cases.OUTPUTS)
        out.append(struct.pack("<4i", C.sizeof(plan), g["channels"], g["frames"], g["L"]) + bytes(plan)
                   + g["mag"].tobytes() + np.ascontiguousarray(g["cw_signal"]).tobytes() + rows)
    with open(sys.argv[1], "wb") as f:
        f.write(struct.pack("<i", len(out)) + b"".join(out))
    print(f"{len(out)} cases")


if __name__ == "__main__":
    main()
