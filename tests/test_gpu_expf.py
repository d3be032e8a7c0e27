"""The device build of ul_expf (uhsdr_amd/csrc/uhsdr_libm_expf.h) pinned on the MI355X itself:
tests/build/libuhsdr_expf_probe.so (tests/device/expf_probe.hip under exactly the product's HIPFLAGS)
evaluates it one thread per operand on the set of tests/expf_cases.py, and every result must equal,
bit for bit (NaN matching NaN), the header's host build, which tests/test_expf.py pins against glibc
on the same set.  The test asserts the count it compared."""
import ctypes as C
import os

import numpy as np
import pytest

import expf_cases
from test_expf import host_probe, run_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1 << 24


def test_device_expf_matches_host_build(cuda):
    import torch                                            # (first: one HIP runtime in the process)
    lib = C.CDLL(os.path.join(ROOT, "tests", "build", "libuhsdr_expf_probe.so"))
    lib.uld_expf.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.uld_expf.restype = C.c_int
    x = expf_cases.operands()
    want = run_host(host_probe().ulh_expf, x).view(np.uint32)
    compared, bad_total, first = 0, 0, None
    for lo in range(0, len(x), CHUNK):
        part = np.ascontiguousarray(x[lo:lo + CHUNK])
        din = torch.from_numpy(part.view(np.int32).copy()).to(cuda)
        dout = torch.empty_like(din)
        err = lib.uld_expf(din.data_ptr(), dout.data_ptr(), len(part), None)
        assert err == 0, f"uld_expf: launch failed with hipError_t {err}"
        got = dout.cpu().numpy().view(np.uint32)
        w = want[lo:lo + len(part)]
        nan = ((got & 0x7fffffff) > 0x7f800000) & ((w & 0x7fffffff) > 0x7f800000)
        bad = np.flatnonzero((got != w) & ~nan)
        compared += len(part)
        bad_total += len(bad)
        if len(bad) and first is None:
            i = int(bad[0])
            first = (float(part[i]).hex(), f"device {int(got[i]):08x}", f"host {int(w[i]):08x}")
    print(f"expf: {bad_total} of {compared} operands differ between device and host build")
    assert compared == expf_cases.COUNT
    assert bad_total == 0, first
