#!/usr/bin/env python3
"""The state streams and expected text of tests/golden/cwtext_*.npz as one raw file, the input of
tools/cwtext/cwdec_sanitize.c (format: see there).  Adds pseudo-random streams, whose expected text
is what the library's host decoder gives (the sanitizer build must agree with the plain one)."""
import glob
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from uhsdr_amd import cwdec  # noqa: E402


def main():
    out = sys.argv[1]
    cases = []
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "cwtext_*.npz"))):
        if p.endswith("chartable.npz"):
            continue
        z = np.load(p)
        cases.append((int(z["blocksize"]), int(z["spikecancel"]), z["state"].astype(np.uint8), z["chars"].astype(np.uint8)))
    rng = np.random.default_rng(11)
    for k, (bs, sc) in enumerate(((8, 0), (72, 2), (128, 1), (40, 2))):
        runs = rng.integers(1, 4 + 5 * k, size=4096)
        state = np.repeat((np.arange(len(runs)) + k) % 2, runs)[:4096].astype(np.uint8)
        d = cwdec.CwDecoder(1, bs, sc, 4096, host=True)
        d.process(np.ascontiguousarray(state[None, :]))
        text, total, _ = d.read()
        assert total[0] <= 4096
        cases.append((bs, sc, state, text[0, :int(total[0])].copy()))
    with open(out, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for bs, sc, state, chars in cases:
            f.write(struct.pack("<4i", bs, sc, len(state), len(chars)))
            f.write(state.tobytes())
            f.write(chars.tobytes())
    print(f"{len(cases)} cases -> {out}")


if __name__ == "__main__":
    main()
