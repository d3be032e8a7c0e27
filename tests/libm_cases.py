"""Operand sets of the libm pin (tests/test_libm.py on the host, tests/test_gpu_libm.py on the device)
and the ctypes access to the two probe libraries the Makefile builds under tests/build.

Every set is a dict: class name -> tuple of uint32 arrays (one per operand of the function), built
in numpy from fixed seeds as bit patterns and cached, so the tests share one copy and never write
to it.  "Neighbourhood of b" is every float within +-4096 ulps of b.  The one set not generated in
numpy is atan2f's "random" class: it is tools/libm_check.c's own generator (a sequential
xorshift64), ported with its seed into the host probe library, so this pin and the exhaustive host
pin of tests/golden/libm_pin.txt see the same pairs."""
import ctypes
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "build")
NEIGH = 4096
INF = 0x7F800000
SIGN = np.uint32(0x80000000)
CHUNK = 1 << 24              # most operands per device launch
FIXTURE_RANDOM = 1 << 14     # operands of a random class kept in tests/golden/libm_device_vectors.npz

# function (the stem of its entry points) -> (number of operands, number of results)
FUNCS = {
    "sincosf": (1, 2),
    "atan2f": (2, 1),
    "atanf_pos": (1, 1),
    "asinf": (1, 1),
    "sqrtf": (1, 1),
    "divf": (2, 1),
    "iq_lowpass": (2, 2),
    "squelch_avg": (2, 1),
}

# operands compared per function: asserted by the tests and recorded in tests/golden/libm_pin.txt
COUNTS = {
    "sincosf": 36_989_710,
    "atan2f": 28_617_234,
    "atanf_pos": 16_904_718,
    "asinf": 16_842_762,
    "sqrtf": 22_300_264,
    "divf": 28_617_234,
    "iq_lowpass": 1_048_576,
    "squelch_avg": 1_048_576,
}


def f2u(x) -> int:
    return int(np.array(x, np.float32).view(np.uint32))


def neighbourhood(b: int, lo: int = 0, hi: int = INF) -> np.ndarray:
    """Bits of every non-negative float within NEIGH ulps of the one with bits b, kept in [lo, hi]."""
    return np.arange(max(b - NEIGH, lo), min(b + NEIGH, hi) + 1, dtype=np.int64).astype(np.uint32)


def both_signs(u: np.ndarray) -> np.ndarray:
    return np.concatenate([u, u | SIGN])


def strided(lo: int, hi: int, stride: int) -> np.ndarray:
    """Bits lo, lo + stride, ... up to hi, and hi itself."""
    u = np.arange(lo, hi + 1, stride, dtype=np.int64)
    if u[-1] != hi:
        u = np.append(u, hi)
    return u.astype(np.uint32)


def _signs(rng, n):
    return rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)


@functools.lru_cache(maxsize=None)
def sincosf_sets():
    rng = np.random.default_rng(0x51C0)
    quad = [neighbourhood(f2u(k * np.pi / 4)) for k in range(1, 9)]
    return _frozen({
        # the header's stated domain (-120, 120)
        "stride61": (both_signs(np.arange(0, f2u(120.0), 61, dtype=np.int64).astype(np.uint32)),),
        "quadrants": (both_signs(np.concatenate(quad)),),           # where n changes
        "tiny_2pi": (both_signs(np.concatenate([neighbourhood(f2u(2.0 ** -12)), neighbourhood(f2u(2 * np.pi))])),),
        "zeros": (np.array([0, 0x80000000], np.uint32),),
        "denormals": (rng.integers(1, 0x00800000, 4096, dtype=np.uint32) | _signs(rng, 4096),),
        # The 631 floats of [2^-12, 120) at which the double that ul_sincosf_poly rounds to the sine or the
        # cosine lies within 2^-20 binary32 ulp of a rounding midpoint (found by a scan of every float of
        # the range): where an error of a few double ulps in the fma chain, the reduction or the
        # int32 conversion shows in the binary32 result at all.  A strided sweep almost never does:
        # such an error moves about one result in 2^29.
        "hard": (both_signs(np.load(os.path.join(HERE, "golden", "libm_sincosf_hard.npy"))),),
    })


ATANF_POINTS = (0x3EE00000, 0x3F300000, 0x3F980000, 0x401C0000, 0x31000000, 0x4C000000, 0x00800000, INF)


@functools.lru_cache(maxsize=None)
def atanf_pos_sets():
    return _frozen({
        "stride127": (strided(0, INF, 127),),
        # fdlibm's reduction boundaries, its 2^-29 and 2^25 cuts, the denormal boundary, +inf from below
        "neighbourhoods": (np.concatenate([neighbourhood(b) for b in ATANF_POINTS]),),
    })


ATAN2_SPECIAL = (0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-30, -1e-30, 3e38, -3e38,
                 1e-45, -1e-45, 0.5, 2.0, 1.5, 0.4375, 1.1875, 2.4375, 0.6875)


@functools.lru_cache(maxsize=None)
def atan2f_sets():
    rng = np.random.default_rng(0xA7A2)
    sp = np.array(ATAN2_SPECIAL, np.float32).view(np.uint32)
    special = (np.repeat(sp, sp.size), np.tile(sp, sp.size))       # tools/libm_check.c's grid, y major

    # every exponent gap -30 .. 30 at every exponent of x (0: denormal), 64 mantissa pairs, 4 sign pairs
    gap, ex = np.meshgrid(np.arange(-30, 31), np.arange(0, 255), indexing="ij")
    ey = ex + gap
    ok = (ey >= 0) & (ey <= 254)
    ex, ey = np.repeat(ex[ok], 64), np.repeat(ey[ok], 64)
    my = rng.integers(0, 1 << 23, ex.size, dtype=np.uint32)
    mx = rng.integers(0, 1 << 23, ex.size, dtype=np.uint32)
    gy = (ey.astype(np.uint32) << np.uint32(23)) | my
    gx = (ex.astype(np.uint32) << np.uint32(23)) | mx
    gaps = (np.concatenate([gy, gy | SIGN, gy, gy | SIGN]), np.concatenate([gx, gx, gx | SIGN, gx | SIGN]))

    n = 2_000_000
    den = (rng.integers(1, 1 << 23, n, dtype=np.uint32) | _signs(rng, n),
           rng.integers(1, 1 << 23, n, dtype=np.uint32) | _signs(rng, n))
    # |y| in [2^-149, 2^-100), |x| in [2^20, 2^128): the quotient underflows; swapped, it overflows
    uy = rng.integers(1, (127 - 100) << 23, n, dtype=np.uint32) | _signs(rng, n)
    ux = rng.integers((127 + 20) << 23, INF, n, dtype=np.uint32) | _signs(rng, n)

    yy = np.arange(0, 1 << 32, 4099, dtype=np.int64).astype(np.uint32)
    one = np.full(yy.size, f2u(1.0), np.uint32)
    return _frozen({
        "special": special,
        "random": host_lib().gen_atan2_pairs(1 << 24),
        "gaps": gaps,
        "denormal": den,
        "underflow": (uy, ux),
        "overflow": (ux, uy),
        "x_one": (np.concatenate([yy, yy]), np.concatenate([one, one | SIGN])),
    })


ASINF_POINTS = (0x32000000, 0x3F000000, 0x3F79999A, 0x3F800000)      # 2^-27, 0.5, 0.975, 1.0 (and past it: NaN)


@functools.lru_cache(maxsize=None)
def asinf_sets():
    return _frozen({
        "stride127": (both_signs(strided(0, 0x3F800000, 127)),),
        "neighbourhoods": (both_signs(np.concatenate([neighbourhood(b) for b in ASINF_POINTS])),),
    })


@functools.lru_cache(maxsize=None)
def sqrtf_sets():
    rng = np.random.default_rng(0x5047)
    # 2^-148 .. 2^-128 (denormal, one bit set) and 2^-126 .. 2^126
    pow4 = [1 << k for k in range(1, 22, 2)] + [e << 23 for e in range(1, 254, 2)]
    # (m 2^e)^2 for a 12-bit m is exact in binary32: that square and its two neighbours
    n = 1 << 20
    root = np.ldexp(rng.integers(1 << 11, 1 << 12, n).astype(np.float32), rng.integers(-70, 51, n).astype(np.int32))
    sq = (root.astype(np.float32) * root.astype(np.float32)).view(np.uint32)
    return _frozen({
        "stride127": (strided(0, INF, 127),),
        "denormals": (np.arange(1, 0x00800000, 7, dtype=np.uint32),),
        "pow4": (np.concatenate([neighbourhood(b) for b in pow4]),),
        "squares": (np.concatenate([sq - np.uint32(1), sq, sq + np.uint32(1)]),),
        "negative_nan": (np.concatenate([
            np.array([0x80000000, 0xBF800000, 0x80000001, 0x807FFFFF, 0xFF800000, 0x7FC00000, 0xFFC00000,
                      0x7F800001, 0x7FFFFFFF], np.uint32),
            rng.integers(1, INF, 4096, dtype=np.uint32) | SIGN]),),
    })


def divf_sets():
    return atan2f_sets()                 # the same classes, read as (a, b)


@functools.lru_cache(maxsize=None)
def mixed_sets():
    """(t, o) of the two mixed-precision recursions: t the new term, o the carried state."""
    rng = np.random.default_rng(0x3D0F)
    n = 1 << 20
    k = n // 4
    anyb = lambda m: rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)      # noqa: E731
    # audio-like magnitudes: |t| up to 2^40 (sums of squares of 32-bit samples), o within 2^+-8 of t / 32
    te = rng.integers(127 - 30, 127 + 40, k, dtype=np.uint32)
    oe = (te.astype(np.int64) - 5 + rng.integers(-8, 9, k)).astype(np.uint32)
    mant = lambda m: rng.integers(0, 1 << 23, m, dtype=np.uint32)                        # noqa: E731
    audio = ((te << np.uint32(23)) | mant(k) | _signs(rng, k), (oe << np.uint32(23)) | mant(k) | _signs(rng, k))
    # denormal o with t = 0, denormal, or just above: the result is rounded to a denormal float
    dt = np.concatenate([np.zeros(k // 2, np.uint32), rng.integers(0, 4 << 23, k - k // 2, dtype=np.uint32)])
    den_o = (dt | _signs(rng, k), rng.integers(1, 1 << 23, k, dtype=np.uint32) | _signs(rng, k))
    # o decaying through the smallest normals
    low = (rng.integers(0, 24 << 23, k, dtype=np.uint32) | _signs(rng, k),
           rng.integers(0, 8 << 23, k, dtype=np.uint32) | _signs(rng, k))
    return _frozen({"any": (anyb(n - 3 * k), anyb(n - 3 * k)), "audio": audio, "denormal_o": den_o, "low": low})


SETS = {
    "sincosf": sincosf_sets,
    "atan2f": atan2f_sets,
    "atanf_pos": atanf_pos_sets,
    "asinf": asinf_sets,
    "sqrtf": sqrtf_sets,
    "divf": divf_sets,
    "iq_lowpass": mixed_sets,
    "squelch_avg": mixed_sets,
}

# classes that are sweeps (not in the fixture) and classes that are random (2^14 operands of each in it);
# every other class -- the special grids and the neighbourhoods -- is in the fixture whole
SWEEPS = {"stride61", "stride127", "x_one"}
RANDOM = {"random", "gaps", "denormal", "underflow", "overflow", "denormals", "squares", "negative_nan",
          "any", "audio", "denormal_o", "low"}


# sub-classes that count as one random class in the fixture: the underflow pairs and their swap, and
# the four magnitude ranges of the (t, o) pairs
FIXTURE_GROUP = {"underflow": "underflow_overflow", "overflow": "underflow_overflow",
                 "any": "pairs", "audio": "pairs", "denormal_o": "pairs", "low": "pairs"}


def fixture_sets(fn: str):
    """The operands of fn recorded in tests/golden/libm_device_vectors.npz: class -> operand tuple.
    A random class is sampled at a fixed stride over its whole length."""
    grouped = {}
    for cls, ops in SETS[fn]().items():
        g = FIXTURE_GROUP.get(cls, cls)
        grouped[g] = ops if g not in grouped else tuple(np.concatenate(p) for p in zip(grouped[g], ops))
    out = {}
    for cls, ops in grouped.items():
        if cls in SWEEPS:
            continue
        if (cls in RANDOM or cls in FIXTURE_GROUP.values()) and ops[0].size > FIXTURE_RANDOM:
            step = ops[0].size // FIXTURE_RANDOM
            ops = tuple(o[::step][:FIXTURE_RANDOM] for o in ops)
        out[cls] = ops
    return out


FIXTURE = os.path.join(HERE, "golden", "libm_device_vectors.npz")


def delta_encode(u: np.ndarray) -> np.ndarray:
    """Results as differences of successive bit patterns (mod 2^32): over a neighbourhood they are
    tiny, so the compressed fixture stays small.  delta_decode inverts it exactly."""
    return np.diff(u.astype(np.uint32), prepend=np.uint32(0))


def delta_decode(d: np.ndarray) -> np.ndarray:
    return np.cumsum(d, dtype=np.uint32)


def operand_crc(ops) -> int:
    import zlib
    crc = 0
    for o in ops:
        crc = zlib.crc32(np.ascontiguousarray(o, "<u4").tobytes(), crc)
    return crc


def count(sets) -> int:
    return sum(ops[0].size for ops in sets.values())


def _frozen(sets):
    for ops in sets.values():
        assert len({o.size for o in ops}) == 1
        for o in ops:
            assert o.dtype == np.uint32
            o.setflags(write=False)
    return sets


# ---- the probe libraries ----

_FP = ctypes.c_void_p


def _lib(name):
    path = os.path.join(BUILD, name)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `make` (build() does) before the libm tests")
    return ctypes.CDLL(path)


class HostProbe:
    """tests/build/libuhsdr_libm_probe_host.so: run(fn, "h" | "g", *operands) -> tuple of uint32 result arrays,
    "h" through the header's host build and "g" through glibc."""

    def __init__(self):
        self.lib = _lib("libuhsdr_libm_probe_host.so")

    def run(self, fn, which, *ops):
        nin, nout = FUNCS[fn]
        assert len(ops) == nin and which in ("h", "g")
        ops = [np.ascontiguousarray(o, np.uint32) for o in ops]
        n = ops[0].size
        outs = [np.empty(n, np.uint32) for _ in range(nout)]
        f = getattr(self.lib, f"ul{which}_{fn}")
        f.argtypes = [_FP] * (nin + nout) + [ctypes.c_size_t]
        f.restype = None
        f(*[a.ctypes.data for a in ops + outs], n)
        return tuple(outs)

    def gen_atan2_pairs(self, n):
        y, x = np.empty(n, np.uint32), np.empty(n, np.uint32)
        f = self.lib.ul_gen_atan2_pairs
        f.argtypes = [ctypes.c_size_t, _FP, _FP]
        f.restype = None
        f(n, y.ctypes.data, x.ctypes.data)
        return y, x


@functools.lru_cache(maxsize=None)
def host_lib() -> HostProbe:
    return HostProbe()


class DeviceProbe:
    """tests/build/libuhsdr_libm_probe.so on cuda:0: run(fn, *operands) -> tuple of uint32 result arrays,
    in launches of at most CHUNK operands on the default stream.  variant="_ieeediv" selects the
    ul_atanf_pos built with UHSDR_ATAN_SHORTDIV 0."""

    def __init__(self, device):
        import torch
        self.torch = torch
        self.device = device
        self.lib = _lib("libuhsdr_libm_probe.so")
        self.launches = 0

    def run(self, fn, *ops, variant=""):
        torch = self.torch
        nin, nout = FUNCS[fn]
        assert len(ops) == nin
        f = getattr(self.lib, f"uld_{fn}{variant}")
        f.argtypes = [_FP] * (nin + nout) + [ctypes.c_size_t, _FP]
        f.restype = ctypes.c_int
        n = ops[0].size
        outs = [np.empty(n, np.uint32) for _ in range(nout)]
        for lo in range(0, n, CHUNK):
            hi = min(lo + CHUNK, n)
            m = hi - lo
            # int32 views: torch has no uint32 arithmetic, and none is needed -- the bits only travel
            din = [torch.from_numpy(np.ascontiguousarray(o[lo:hi]).view(np.int32).copy()).to(self.device) for o in ops]
            dout = [torch.empty(m, dtype=torch.int32, device=self.device) for _ in range(nout)]
            err = f(*[t.data_ptr() for t in din + dout], m, None)
            assert err == 0, f"uld_{fn}{variant}: launch failed with hipError_t {err}"
            self.launches += 1
            for o, t in zip(outs, dout):
                o[lo:hi] = t.cpu().numpy().view(np.uint32)
        return tuple(outs)


# ---- comparison ----

def _nan(u):
    return (u & np.uint32(0x7FFFFFFF)) > np.uint32(INF)


def differing(a, b) -> np.ndarray:
    """Indices where any result of a differs from b's: bit for bit, two NaNs equal whatever their payload."""
    bad = np.zeros(a[0].size, bool)
    for x, y in zip(a, b):
        bad |= (x != y) & ~(_nan(x) & _nan(y))
    return np.flatnonzero(bad)


def hexf(u) -> str:
    return float(np.array(u, np.uint32).view(np.float32)).hex() + f" [0x{int(u):08x}]"


def report(fn, cls, ops, i, named, nbad, n) -> str:
    """fn's failure text: the first differing operand and every named result at it, as hex floats."""
    args = ", ".join(hexf(o[i]) for o in ops)
    vals = "; ".join(f"{name} " + " ".join(hexf(r[i]) for r in res) for name, res in named)
    return f"{fn}({args}) [class {cls}]: {vals}; {nbad} of {n} operands differ"
