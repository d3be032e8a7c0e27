"""The operand set of the expf pins (tests/test_expf.py: the header's host build against glibc;
tests/test_gpu_expf.py: the device build against the host build), built once and shared, read-only:

  * every binary32 within 4096 ulps of +0 and -0, of +-1, of +-88 (where the special-case branch
    begins), of the overflow threshold 0x1.62e42ep6 and of the two underflow thresholds
    -0x1.9fe368p6 and -0x1.9d1d9ep6, and of k * ln2 / 64 for k = +-1 .. +-64 (the edges of the
    reduction's intervals, where k of 2^(k/32) changes and r is largest)
  * every 127th binary32 of the whole range, infinities and NaNs included
  * 2^20 random negative operands, the noise reduction's argument range (xih1r * X / xt < 0),
    log-uniform in magnitude from 1e-6 to 200

COUNT is fixed here, not derived from the arrays: 135 neighbourhoods of 8193 and the two of a zero
of 4097 (the magnitude does not go below 0), ceil(2^32 / 127) strided operands, 2^20 random ones."""
import functools

import numpy as np

ULPS = 4096
COUNT = 135 * 8193 + 2 * 4097 + 33818641 + (1 << 20)        # 35981466


def _around(center):
    b = int(np.float32(center).view(np.uint32))
    sign, mag = b & 0x80000000, b & 0x7fffffff
    m = np.arange(max(0, mag - ULPS), mag + ULPS + 1, dtype=np.int64)
    return (m | sign).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def operands():
    centers = [0.0, -0.0, 1.0, -1.0, 88.0, -88.0, float.fromhex("0x1.62e42ep6"), float.fromhex("-0x1.9fe368p6"),
               float.fromhex("-0x1.9d1d9ep6")]
    centers += [s * k * np.log(2.0) / 64.0 for k in range(1, 65) for s in (1.0, -1.0)]
    parts = [_around(c) for c in centers]
    parts.append(np.arange(0, 1 << 32, 127, dtype=np.int64).astype(np.uint32))
    rng = np.random.default_rng(1212)
    parts.append((-np.exp(rng.uniform(np.log(1e-6), np.log(200.0), 1 << 20))).astype(np.float32).view(np.uint32))
    x = np.concatenate(parts).view(np.float32)
    x.setflags(write=False)
    return x
