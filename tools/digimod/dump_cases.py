#!/usr/bin/env python3
"""Write the modulator fixtures (tests/golden/digimod_*.npz) as one flat file for
tools/digimod/digimod_sanitize.c:

  int32 cases, then per case
    int32 kind (0 rtty, 1 psk), shift_idx, speed_idx, stopbits_idx, capacity, total, blocks, ops
    uint32 consumed, txoff_at, state after the last gen
    uint32 crc [blocks]       crc32 of every block of 1024 samples (the last one shorter)
    per op: int32 type (0 put, 1 gen, 2 start), int32 arg (bytes, samples, 0), the bytes of a put

  python3 tools/digimod/dump_cases.py /tmp/digimod_cases.bin
"""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from digimod_cases import BLOCK, CASES, load_case  # noqa: E402


def main():
    with open(sys.argv[1], "wb") as f:
        f.write(np.int32(len(CASES)).tobytes())
        for name in CASES:
            g = load_case(name)
            if "samples" in g:
                crc = np.array([zlib.crc32(g["samples"][k:k + BLOCK].tobytes()) for k in range(0, g["total"], BLOCK)], np.uint32)
            else:
                crc = g["block_crc"]
            f.write(np.array([g["kind"] == "psk", g["shift_idx"], g["speed_idx"], g["stopbits_idx"], g["capacity"], g["total"],
                              len(crc), len(g["ops"])], np.int32).tobytes())
            f.write(np.array([g["consumed"][-1], g["txoff_at"][-1], g["state"][-1]], np.uint32).tobytes())
            f.write(crc.astype(np.uint32).tobytes())
            for op in g["ops"]:
                if op[0] == "put":
                    f.write(np.array([0, len(op[1])], np.int32).tobytes() + op[1])
                else:
                    f.write(np.array([1, op[1]] if op[0] == "gen" else [2, 0], np.int32).tobytes())
    print(f"{len(CASES)} cases -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
