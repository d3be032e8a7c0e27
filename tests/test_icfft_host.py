"""The host restatement of arm_cfft_f32(&arm_cfft_sR_f32_len256, x, 1, 1) (uhsdr_cfft.h cfft256_host,
the transform of the noise reduction's host twin) against inverse transforms recorded from the
reference (tests/golden/nr_icfft.npz, tools/nr/make_nr_golden.py): an impulse, a conjugate-symmetric
spectrum, a conjugate-asymmetric one, a single bin, and values over 60 decades with a negative zero.
Exact."""
import ctypes as C
import os

import numpy as np

import uhsdr_amd as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cfft(x, inverse):
    y = np.ascontiguousarray(x, dtype=np.float32).copy()
    U._abi.check(U.load().uhsdr_nr_cfft256_host(y.ctypes.data_as(C.c_void_p), int(inverse)), "uhsdr_nr_cfft256_host")
    return y


def test_inverse_transform_matches_the_reference():
    z = np.load(os.path.join(GOLDEN, "nr_icfft.npz"))
    x, y = z["x"], z["y"]
    assert x.shape == (5, 512) and y.shape == (5, 512)
    c = x.view(np.complex64)
    assert np.array_equal(c[1, 1:128], np.conj(c[1, :128:-1]))             # symmetric: a real signal
    assert not np.array_equal(c[2, 1:128], np.conj(c[2, :128:-1]))         # asymmetric
    assert np.abs(y[1, 1::2]).max() < 1e-5 and np.abs(y[2, 1::2]).max() > 1
    for k in range(len(x)):
        got = cfft(x[k], True)
        assert np.array_equal(got.view(np.uint32), y[k].view(np.uint32)), k
    # against the definition, loosely: the recording is an inverse DFT
    ref = np.fft.ifft(c[2].astype(np.complex128))
    assert np.abs(y[2].view(np.complex64) - ref).max() < 1e-3


def test_forward_then_inverse_returns_the_input():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(512).astype(np.float32)
    back = cfft(cfft(x, False), True)
    assert np.abs(back - x).max() < 1e-5
    ref = np.fft.fft(x.view(np.complex64).astype(np.complex128))
    assert np.abs(cfft(x, False).view(np.complex64) - ref).max() < 1e-3
