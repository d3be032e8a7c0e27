"""uhsdr_amd/csrc/uhsdr_libm.h (the device's sincosf / atan2f) reproduces the host glibc bit for
bit -- the SAM PLL and FM discriminator of the reference call glibc (audio_driver.c:2039,
2128, 1581).  tools/libm_check.c is compiled here and run on a strided subset (every 251st
float of [-2pi, 2pi]) and on 2e6 atan2f operand pairs; the exhaustive run (every float of
[-2pi, 2pi], 2e8 atan2f pairs) is recorded in tests/golden/libm_pin.txt.

The second half runs the header's host build (tests/build/libuhsdr_libm_probe_host.so) against glibc on
the operand sets of tests/libm_cases.py: the reference leg of the device pin, tests/test_gpu_libm.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import libm_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "libm_check")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "libm_check.c"), "-lm"],
                   check=True)
    return exe


def test_sincosf_matches_glibc(tmp_path):
    r = subprocess.run([_build(tmp_path), "sincos", "251"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert " 0 of " in r.stdout


def test_atan2f_matches_glibc(tmp_path):
    r = subprocess.run([_build(tmp_path), "atan2", "2000000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert " 0 of " in r.stdout


def test_atan2f_x_one_matches_glibc(tmp_path):
    """atan2f(y, 1) -- fdlibm's atanf(y) case, which the branch-free ul_atan2f folds into its main
    path: every 4099th binary32 y here, every y in the exhaustive run (libm_pin.txt)."""
    r = subprocess.run([_build(tmp_path), "atan2x1", "4099"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert " 0 of " in r.stdout


def test_atanf_nonnegative_matches_glibc(tmp_path):
    """ul_atanf_pos, atan2f's reduction of |y / x|: every 1021st float of [0, inf] here, every one in
    the exhaustive run (libm_pin.txt)."""
    r = subprocess.run([_build(tmp_path), "atanpos", "1021"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert " 0 of " in r.stdout


def test_asinf_matches_glibc(tmp_path):
    """The twin-peaks detector's asinf (audio_driver.c:2211); exhaustive run in libm_pin.txt."""
    r = subprocess.run([_build(tmp_path), "asin", "127"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert " 0 of " in r.stdout


# ---- the operand sets of the device pin (tests/libm_cases.py, tests/test_gpu_libm.py) on the host ----

def _host_differences(fn, sets, reference, ref_name):
    host = L.host_lib()
    n, fails = 0, []
    for cls, ops in sets.items():
        h = host.run(fn, "h", *ops)
        r = reference(cls, ops)
        n += ops[0].size
        bad = L.differing(h, r)
        if bad.size:
            fails.append(L.report(fn, cls, ops, bad[0], [("host header", h), (ref_name, r)], bad.size, ops[0].size))
    return n, fails


@pytest.mark.parametrize("fn", list(L.FUNCS))
def test_header_matches_glibc_on_device_sets(fn):
    """The reference leg of the device pin: on every operand that tests/test_gpu_libm.py presents to the
    device, the header's host build (tests/build/libuhsdr_libm_probe_host.so, HOSTCFLAGS) equals glibc,
    bit for bit with NaN matching NaN.

    What the sets catch was tried on this leg with mutated scratch copies of the header (none
    committed), each built like the host probe; "a/b" is operands differing of operands in the class.
      last bit of one aT coefficient of ul_atanf_pos:
        aT[0] + 1 ulp   atan2f random 42252/16777216, gaps 2474/3744000, denormal 7635/2000000,
                        x_one 318/2095618; atanf_pos stride127 4033/16843270, neighbourhoods 421/61448
        aT[4] + 1 ulp   atan2f random 3/16777216, denormal 1/2000000
        aT[10] + 1 ulp  not caught
      one reduction boundary by one ulp (exactly one operand per sign changes branch, and every
      such operand is in a neighbourhood class):
        ul_atanf_pos lo2 0x3f980000 + 1   atanf_pos neighbourhoods 1/61448, atan2f special 1/400
        ul_atanf_pos 2^25 cut - 1         atanf_pos neighbourhoods 1/61448
        ul_asinf 0.5 cut - 1              asinf neighbourhoods 2/65544
        ul_sincosf n: 0x800000 + 1        sincosf quadrants 1/131088
        not caught, because both branches give the same binary32 at the one operand that moves:
        ul_atanf_pos 0x3ee00000 +-1, 0x3f300000 +-1, 0x3f980000 - 1, 0x401c0000 +-1, 0x31000000 + 1;
        ul_asinf 0x3F79999A +-1, 0x3f000000 + 1, 0x32000000 + 1; ul_atan2f's k cuts at 25 / 27
      fused multiply-add of the double chain as a multiply and an add:
        fma(x5, s1, s)           not caught, and cannot be: compared over every float of [2^-12, 120)
                                 the mutant returns the same binary32 sine and cosine as the header
                                 (the two differ by a double ulp, about 2^-29 binary32 ulp); the same
                                 holds for each of the other polynomial fma calls
        fma(-n, hpi, x)          sincosf hard 10/1262 (17 floats of the whole range differ)
        hpi + 1 double ulp       sincosf hard 22/1262, quadrants 2/131088
      The "hard" class exists because of this: the strided sweep caught neither of the last two."""
    host = L.host_lib()
    n, fails = _host_differences(fn, L.SETS[fn](), lambda cls, ops: host.run(fn, "g", *ops), "glibc")
    assert not fails, "\n".join(fails)
    assert n == L.COUNTS[fn]


@pytest.mark.parametrize("fn", list(L.FUNCS))
def test_header_matches_recorded_glibc(fn):
    """The header's host build against tests/golden/libm_device_vectors.npz, glibc 2.35's recorded
    results on the fixture operands: the header's arithmetic is the same on any host, so this holds
    whatever libm the machine has, and it checks that the operand generator still gives the operands
    the results were recorded for."""
    z = np.load(L.FIXTURE)
    man = json.loads(str(z["manifest"]))[fn]
    sets = L.fixture_sets(fn)
    assert set(sets) == set(man)
    for cls, ops in sets.items():
        assert man[cls] == {"count": ops[0].size, "crc32": L.operand_crc(ops)}, f"{fn}.{cls}: operands changed"
    nout = L.FUNCS[fn][1]
    n, fails = _host_differences(fn, sets, lambda cls, ops: tuple(L.delta_decode(z[f"{fn}.{cls}.r{j}"]) for j in range(nout)),
                                 "recorded glibc 2.35")
    assert not fails, "\n".join(fails)
    assert n == sum(c["count"] for c in man.values())


def test_atan2_pairs_are_libm_check_pairs(tmp_path):
    """libm_cases' "special" and "random" atan2f classes are the pairs tools/libm_check.c itself draws
    ("pairs" prints what "atan2" checks), so the device pin and the exhaustive host pin of
    tests/golden/libm_pin.txt see the same operands."""
    count = 1 << 16
    r = subprocess.run([_build(tmp_path), "pairs", str(count)], capture_output=True, timeout=120)
    assert r.returncode == 0
    yx = np.frombuffer(r.stdout, "<u4").reshape(-1, 2)
    sets = L.atan2f_sets()
    want = np.concatenate([np.stack(sets["special"], 1), np.stack(sets["random"], 1)[:count]])
    assert yx.shape == want.shape == (400 + count, 2)
    assert np.array_equal(yx, want)


def test_pin_file_records_the_counts_compared():
    """tests/golden/libm_pin.txt's line for the device run carries the operand counts the tests assert."""
    line = [l for l in open(os.path.join(ROOT, "tests", "golden", "libm_pin.txt")) if l.startswith("device build")][-1]
    for fn, n in L.COUNTS.items():
        assert f"0 of {n}" in line, fn
    assert f"0 of {sum(L.count(L.fixture_sets(fn)) for fn in L.FUNCS)} fixture operands" in line
