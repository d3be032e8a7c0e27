"""ul_expf (uhsdr_amd/csrc/uhsdr_libm_expf.h), the host build, against the host's glibc expf bit for bit
on the operand set of tests/expf_cases.py -- the noise reduction's speech-presence probability calls
expf per bin and frame (audio_nr.c:2010) and feeds the result back into its noise estimate.  The
exhaustive run over all 2^32 operands (tools/libm_check expf 1) is recorded in
tests/golden/expf_pin.txt."""
import ctypes as C
import os

import numpy as np

import expf_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_probe():
    lib = C.CDLL(os.path.join(ROOT, "tests", "build", "libuhsdr_expf_probe_host.so"))
    for name in ("ulh_expf", "ulg_expf"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        getattr(lib, name).restype = None
    return lib


def run_host(fn, x):
    r = np.empty_like(x)
    fn(x.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), len(x))
    return r


def test_expf_matches_glibc():
    lib = host_probe()
    x = expf_cases.operands()
    ours, glibc = run_host(lib.ulh_expf, x), run_host(lib.ulg_expf, x)
    diff = np.flatnonzero(ours.view(np.uint32) != glibc.view(np.uint32))
    print(f"expf: {len(diff)} of {len(x)} operands differ from glibc")
    assert len(x) == expf_cases.COUNT
    assert len(diff) == 0, [(float(x[i]).hex(), float(glibc[i]).hex(), float(ours[i]).hex()) for i in diff[:10]]


def test_expf_special_cases():
    """the branches the noise reduction can reach (0 / 0 gives NaN, X / 0 gives -inf) and the others"""
    lib = host_probe()
    x = np.array([-np.inf, np.inf, np.nan, -np.nan, -0.0, 0.0, 89.0, -104.0, -103.5, -103.0, -87.5, 88.7, 88.8], np.float32)
    r = run_host(lib.ulh_expf, x)
    assert r[0] == 0 and not np.signbit(r[0]) and r[1] == np.inf and np.isnan(r[2]) and np.isnan(r[3])
    assert r[4] == 1 and r[5] == 1 and r[6] == np.inf and r[7] == 0
    assert r[8].view(np.uint32) == 1 and r[9].view(np.uint32) == 1          # the smallest denormal, two ways
    assert np.isfinite(r[11]) and r[12] == np.inf
    assert np.array_equal(r.view(np.uint32), run_host(lib.ulg_expf, x).view(np.uint32))


def test_exhaustive_run_is_recorded():
    text = open(os.path.join(ROOT, "tests", "golden", "expf_pin.txt")).read()
    assert "0 of 4294967296 arguments differ" in text
