#!/usr/bin/env python3
"""Write the noise-blanker frame fixtures with their regenerated inputs into one binary file for
tools/nb/nb_sanitize.c:

  python3 tools/nb/dump_cases.py /tmp/nb_cases.bin

File: int32 count, then per case int32 nb_setting, int32 samples, float32 audio[samples], float32
out[samples]."""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nb_cases  # noqa: E402


def main():
    out = []
    for name in nb_cases.CASES:
        g = nb_cases.load_case(name)
        out.append(struct.pack("<ii", g["cfg"]["nb_setting"], len(g["out"])) + g["audio"].tobytes() + g["out"].tobytes())
    with open(sys.argv[1], "wb") as f:
        f.write(struct.pack("<i", len(out)) + b"".join(out))
    print(f"{len(out)} cases")


if __name__ == "__main__":
    main()
