#!/usr/bin/env python3
"""Write the CW generator fixtures (tests/golden/cwgen_*.npz) as one flat file for
tools/cwgen/cwgen_sanitize.c:

  int32 cases, then per case
    int32 mode, speed, weight, reverse, rx_delay, sidetone, capacity, blocks, events, echo bytes
    uint32 consumed
    uint8 keys [blocks], uint8 flags [blocks], uint32 i_crc [blocks], uint32 q_crc [blocks], uint8 echo []
    per event: int32 block, type (0 put, 1 speed), a, b (put: bytes, 0; speed: wpm, weight), the bytes of a put

  python3 tools/cwgen/dump_cases.py /tmp/cwgen_cases.bin
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from cwgen_cases import CASES, SETTINGS, load_case  # noqa: E402


def main():
    with open(sys.argv[1], "wb") as f:
        f.write(np.int32(len(CASES)).tobytes())
        for name in CASES:
            g = load_case(name)
            f.write(np.array([g[k] for k in SETTINGS] + [g["blocks"], len(g["events"]), len(g["echo"])], np.int32).tobytes())
            f.write(np.uint32(g["consumed"]).tobytes())
            f.write(g["keys"].tobytes() + g["flags"].tobytes() + g["i_crc"].tobytes() + g["q_crc"].tobytes() + g["echo"])
            for b, op in g["events"]:
                if op[0] == "put":
                    f.write(np.array([b, 0, len(op[1]), 0], np.int32).tobytes() + op[1])
                else:
                    f.write(np.array([b, 1, op[1], op[2]], np.int32).tobytes())
    print(f"{len(CASES)} cases -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
