#!/usr/bin/env python3
"""Write the noise-reduction fixtures with their regenerated inputs into one binary file for
tools/nr/nr_sanitize.c:

  python3 tools/nr/dump_cases.py /tmp/nr_cases.bin

File: int32 count, then per case int32 kind (0 frames, 1 stream), the uhsdr_nr_config as float32 alpha
and int32 asnr, width, power_threshold_int, width_hz, offset_hz, sample_rate, then int32 samples, int32
reset (the frame before which the run restarts, or -1), float32 audio[samples], float32 out[samples].
Cases kept as a crc32 per frame (the long ones) are left out."""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nr_cases  # noqa: E402


def main():
    out = []
    for kind, names, load in ((0, nr_cases.CASES, nr_cases.load_case), (1, nr_cases.STREAM_CASES, nr_cases.load_stream_case)):
        for name in names:
            g = load(name)
            if "out" not in g:
                continue
            c = g["cfg"]
            y = np.ascontiguousarray(g["out"], dtype=np.float32).reshape(-1)
            head = struct.pack("<if6iii", kind, c["alpha"], c["asnr"], c["width"], c["power_threshold_int"], c["width_hz"], c["offset_hz"],
                               c["sample_rate"], len(y), int(g["reset"]) if kind == 0 else -1)
            out.append(head + g["audio"][:len(y)].tobytes() + y.tobytes())
    with open(sys.argv[1], "wb") as f:
        f.write(struct.pack("<i", len(out)) + b"".join(out))
    print(f"{len(out)} cases")


if __name__ == "__main__":
    main()
