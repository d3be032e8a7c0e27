"""The device build of uhsdr_amd/csrc/uhsdr_libm.h, and the IEEE primitives the chain assumes, pinned
on the MI355X itself.

tests/build/libuhsdr_libm_probe.so (tests/device/libm_probe.hip under exactly the product's HIPFLAGS)
evaluates ul_sincosf, ul_atan2f, ul_atanf_pos (with the short division, and with the IEEE quotient),
ul_asinf, sqrtf, binary32 '/', and the two mixed-precision recursions, one thread per operand, on
every operand of the sets of tests/libm_cases.py.  Each result must equal, bit for bit (NaN matching
NaN), the header's host build, which tests/test_libm.py pins against glibc on the same sets; and, on
the fixture operands, the results glibc 2.35 gave when tests/golden/libm_device_vectors.npz was
recorded.  No operand is left out: each test asserts the count it compared (libm_cases.COUNTS, the
figures of tests/golden/libm_pin.txt)."""
import json

import numpy as np
import pytest

import libm_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(cuda):
    return L.DeviceProbe(cuda)


def compare(fn, sets, device, reference, ref_name):
    """device(ops) against reference(cls, ops) on every class of sets; returns (operands compared, failure texts)."""
    host = L.host_lib()
    n, fails = 0, []
    for cls, ops in sets.items():
        d = device(ops)
        r = reference(cls, ops)
        assert all(x.size == ops[0].size for x in d + r)
        n += ops[0].size
        bad = L.differing(d, r)
        if bad.size:
            i = bad[0]
            one = tuple(o[i:i + 1] for o in ops)
            named = [("device", tuple(x[i:i + 1] for x in d)), (ref_name, tuple(x[i:i + 1] for x in r)),
                     ("host header", host.run(fn, "h", *one)), ("this host's glibc", host.run(fn, "g", *one))]
            fails.append(L.report(fn, cls, one, 0, named, bad.size, ops[0].size))
    return n, fails


@pytest.mark.parametrize("fn", list(L.FUNCS))
def test_device_matches_host_build(dev, fn):
    """Every operand of fn's sets: the device result equals the header's host build."""
    host = L.host_lib()
    before = dev.launches
    n, fails = compare(fn, L.SETS[fn](), lambda ops: dev.run(fn, *ops),
                       lambda cls, ops: host.run(fn, "h", *ops), "host header")
    assert not fails, "\n".join(fails)
    assert n == L.COUNTS[fn]
    assert dev.launches - before >= -(-n // L.CHUNK)


def test_atanf_pos_short_division(dev):
    """ul_atanf_pos as the kernels get it (v_rcp_f32 and one residual correction) against the same
    function with the IEEE quotient, both on the device, and the latter against the host build: a
    difference in the first comparison alone is the short division's."""
    host = L.host_lib()
    sets = L.atanf_pos_sets()
    ieee = {cls: dev.run("atanf_pos", *ops, variant="_ieeediv") for cls, ops in sets.items()}
    n, fails = compare("atanf_pos", sets, lambda ops: dev.run("atanf_pos", *ops),
                       lambda cls, ops: ieee[cls], "device, IEEE quotient")
    m, fails2 = compare("atanf_pos", sets, lambda ops: dev.run("atanf_pos", *ops, variant="_ieeediv"),
                        lambda cls, ops: host.run("atanf_pos", "h", *ops), "host header")
    assert not fails + fails2, "\n".join(["short division vs IEEE quotient:"] + fails + ["IEEE quotient vs host:"] + fails2)
    assert n == m == L.COUNTS["atanf_pos"]
    # every 127th float of [7/16, 2^25) reached the division
    a = sets["stride127"][0]
    assert np.count_nonzero((a >= 0x3EE00000) & (a < 0x4C000000)) == 1_733_866


@pytest.mark.parametrize("fn", list(L.FUNCS))
def test_device_matches_recorded_glibc(dev, fn):
    """The special grids, every neighbourhood and 2^14 operands of each random class against the results
    recorded from glibc 2.35 (tests/golden/make_libm_vectors.py): independent of this host's libm."""
    z = np.load(L.FIXTURE)
    man = json.loads(str(z["manifest"]))[fn]
    sets = L.fixture_sets(fn)
    assert set(sets) == set(man)
    for cls, ops in sets.items():
        assert man[cls] == {"count": ops[0].size, "crc32": L.operand_crc(ops)}, f"{fn}.{cls}: operands changed"
    nout = L.FUNCS[fn][1]
    n, fails = compare(fn, sets, lambda ops: dev.run(fn, *ops),
                       lambda cls, ops: tuple(L.delta_decode(z[f"{fn}.{cls}.r{j}"]) for j in range(nout)),
                       "recorded glibc 2.35")
    assert not fails, "\n".join(fails)
    assert n == sum(c["count"] for c in man.values())
