"""Shared helpers of the edge-input tests (tests/golden/rxedge_*.npz, txedge_*.npz; see
make_golden.py EDGE_CONFIGS): load a fixture with its input regenerated and the conditions that
give it its point checked, and compare outputs with its per-call crc32s and stored windows."""
import functools
import glob
import json
import os
import zlib

import numpy as np

import oracle
import uhsdr_amd as U
from uhsdr_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RX_NAMES = sorted(os.path.basename(f)[7:-4] for f in glob.glob(os.path.join(GOLDEN, "rxedge_*.npz")))
TX_NAMES = sorted(os.path.basename(f)[7:-4] for f in glob.glob(os.path.join(GOLDEN, "txedge_*.npz")))
WINDOWS = (4096, 2048, 6144)          # head, from the first denormal, tail
FLT_MIN = np.float32(1.17549435e-38)
MODE_AM, MODE_SAM = 3, 4              # uhsdr_ref mode= of the configs whose output never goes denormal


def denormals(x) -> int:
    a = np.abs(x)
    return int(((a > 0) & (a < FLT_MIN)).sum())


def call_crcs(x: np.ndarray) -> np.ndarray:
    """crc32 of every 32-frame call of x [n, ...]"""
    b = np.ascontiguousarray(x).reshape(x.shape[0] // 32, -1).view(np.uint8)
    return np.array([zlib.crc32(r) for r in b], np.uint32)


@functools.lru_cache(maxsize=None)
def load_rx(name: str) -> dict:
    """The fixture's arrays, `kinds`, `args`, `base` (the generator), `base_kw`, `stereo` (a_buffer[0]
    recorded on its own) and `rows`, the regenerated input int32 [kinds][frames][2], read-only."""
    z = np.load(os.path.join(GOLDEN, f"rxedge_{name}.npz"), allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["name"] = name
    g["kinds"] = json.loads(str(g["kinds"]))
    g["args"] = json.loads(str(g["args"]))
    g["base_kw"] = json.loads(str(g["base_kw"]))
    g["base"] = getattr(synth, str(g["base"]))
    g["frames"] = n = int(g["frames"])
    g["stereo"] = "crc_a0" in g
    assert tuple(g["kinds"]) == synth.EDGE_KINDS and n == synth.EDGE_FRAMES
    rows = np.stack([synth.edge_iq(k, [0], 0, n, base=g["base"], **g["base_kw"])[0] for k in g["kinds"]])
    crc = [zlib.crc32(np.ascontiguousarray(r).tobytes()) for r in rows]
    assert crc == g["iq_crc32"].tolist(), f"rxedge_{name}: synth.edge_iq drifted"
    rows.setflags(write=False)
    g["rows"] = rows
    # what the fixture is for
    assert not g["nonfinite"].any() and np.isfinite(g["win_a1"]).all(), f"rxedge_{name}: non-finite output"
    if g["args"]["mode"] not in (MODE_AM, MODE_SAM):
        for kind in ("burst", "impulse"):
            d = int(g["denormal_a1"][g["kinds"].index(kind)])
            assert d >= 20000, f"rxedge_{name} {kind}: only {d} denormal a1 samples"
    if name == "p48_agcoff":
        for kind in ("rails", "lowbits"):
            p = float(g["peak_a1"][g["kinds"].index(kind)])
            assert p > 32768, f"rxedge_{name} {kind}: peak |a1| {p} does not wrap the codec frames"
    return g


@functools.lru_cache(maxsize=None)
def load_tx(name: str) -> dict:
    z = np.load(os.path.join(GOLDEN, f"txedge_{name}.npz"), allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["name"] = name
    g["kinds"] = json.loads(str(g["kinds"]))
    g["args"] = json.loads(str(g["args"]))
    g["frames"] = n = int(g["frames"])
    assert tuple(g["kinds"]) == synth.EDGE_AUDIO_KINDS and n == synth.EDGE_AUDIO_FRAMES
    rows = np.stack([synth.edge_audio(k, [0], 0, n)[0] for k in g["kinds"]])
    crc = [zlib.crc32(np.ascontiguousarray(r).tobytes()) for r in rows]
    assert crc == g["audio_crc32"].tolist(), f"txedge_{name}: synth.edge_audio drifted"
    rows.setflags(write=False)
    g["rows"] = rows
    assert not g["nonfinite"].any() and np.isfinite(g["win_a0"]).all(), f"txedge_{name}: non-finite output"
    d = int(g["denormal_a0"][g["kinds"].index("burst")])
    assert d >= 50000, f"txedge_{name} burst: only {d} denormal a0 samples"
    return g


def rx_config(g):
    return U.config_from_ref_args(g["args"])


def tx_config(g):
    return U.tx_config_from_ref_args(g["args"])


def mismatch(g, r: int, outs: dict, frame0: int = 0):
    """Compare row r's outputs -- outs: {"a1" | "a0" | "dst" | "iq": array covering frames frame0 ..},
    a whole number of 32-frame calls -- with the fixture's crc32 per call and with its stored
    windows where they overlap.  Returns None, or (32-frame call, key, text) of the first call that
    differs."""
    worst = None
    for key, x in outs.items():
        if x is None:
            continue
        ckey = "crc_a1" if key == "a0" and not g.get("stereo", True) else f"crc_{key}"
        c0 = frame0 // 32
        got = call_crcs(x)
        bad = np.flatnonzero(got != g[ckey][r, c0:c0 + len(got)])
        if len(bad) and (worst is None or c0 + bad[0] < worst[0]):
            worst = (int(c0 + bad[0]), key, f"{len(bad)} of {len(got)} calls differ")
    if worst is not None:
        return worst
    for key, x in outs.items():          # the crcs agree: the windows must too
        wkey = "win_a1" if key == "a0" and not g.get("stereo", True) else f"win_{key}"
        if x is None or wkey not in g:
            continue
        off = 0
        for s, w in zip(g["win_start"][r], WINDOWS):
            lo, hi = max(int(s), frame0), min(int(s) + w, frame0 + len(x))
            if lo < hi:
                a = np.ascontiguousarray(x[lo - frame0:hi - frame0])
                b = np.ascontiguousarray(g[wkey][r, off + lo - int(s):off + hi - int(s)])
                if a.tobytes() != b.tobytes():
                    return (lo // 32, key, "stored window differs though the crcs agree")
            off += w
    return None


def oracle_rx_call(g, r: int, call: int):
    """the oracle's (a1, a0, dst) of row r's 32-frame call `call` (pinned to the reference by
    test_edge_oracle.py), for a failure message"""
    o = oracle.OracleRx(U.build_plan(rx_config(g)), 1)
    a1, a0, dst = o.process2(np.ascontiguousarray(g["rows"][r:r + 1, :32 * (call + 1)]))
    return a1[0, -32:], a0[0, -32:], dst[0, -32:]


def describe(g, r: int, lane, bad, got: dict, frame0: int = 0) -> str:
    """failure text: lane, call, the device's and the oracle's samples of that call"""
    call, key, text = bad
    ref = dict(zip(("a1", "a0", "dst"), oracle_rx_call(g, r, call))) if "iq" not in got else {}
    lo = 32 * call - frame0
    dev = np.asarray(got[key][lo:lo + 32]).ravel()
    at = 0
    if key in ref:                       # show the samples from the first one that differs
        ne = np.flatnonzero(dev.view(np.uint32) != ref[key].ravel().view(np.uint32))
        at = int(ne[0]) if len(ne) else 0
    lines = [f"rxedge_{g['name']} row {g['kinds'][r]} lane {lane}: first differing call {call} "
             f"(frames {32 * call}..{32 * call + 31}) in {key}; {text}",
             f"  device {key}[{at}:]: {dev[at:at + 8]!r}"]
    if key in ref:
        lines.append(f"  oracle {key}[{at}:]: {ref[key].ravel()[at:at + 8]!r}")
    return "\n".join(lines)
