#!/usr/bin/env python3
"""Generate tests/golden/libm_device_vectors.npz: glibc's own results (sincosf, atan2f, atanf, asinf,
sqrtf, '/', and the two mixed-precision recursions in plain C) on the fixture operands of
tests/libm_cases.py -- the special grids, every neighbourhood set and 2^14 operands of each random
class.  tests/test_gpu_libm.py compares the device with these, so that leg does not depend on the
libm of the machine the GPU is in.

Run it on a host whose libm is the one the project pins (glibc 2.35), after `make`:

    python tests/golden/make_libm_vectors.py

The operands are not stored: libm_cases regenerates them from its seeds, and each class's crc32 is
stored to catch a generator that drifts.  Results are stored as differences of successive bit
patterns (libm_cases.delta_encode), written with fixed zip timestamps, so a rerun reproduces the
committed bytes."""
import json
import os
import platform
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import libm_cases as L  # noqa: E402
from make_golden import save_npz  # noqa: E402


def main():
    host = L.host_lib()
    arrays, manifest = {}, {}
    for fn in L.FUNCS:
        manifest[fn] = {}
        for cls, ops in L.fixture_sets(fn).items():
            res = host.run(fn, "g", *ops)
            manifest[fn][cls] = {"count": int(ops[0].size), "crc32": L.operand_crc(ops)}
            for j, r in enumerate(res):
                arrays[f"{fn}.{cls}.r{j}"] = L.delta_encode(r)
    manifest["libc"] = " ".join(platform.libc_ver())
    arrays["manifest"] = np.array(json.dumps(manifest, sort_keys=True))
    save_npz(L.FIXTURE, **arrays)
    total = sum(c["count"] for fn in L.FUNCS for c in manifest[fn].values())
    print(f"{L.FIXTURE}: {total} operands, {os.path.getsize(L.FIXTURE)} bytes, {manifest['libc']}")


if __name__ == "__main__":
    main()
