"""Loader and runner of the CW generator fixtures (tests/golden/cwgen_*.npz, recorded from the
reference firmware by tools/cwgen/make_cwgen_golden.py)."""
import glob
import json
import os
import zlib

import numpy as np

from uhsdr_amd import cwgen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(n for n in (os.path.basename(p)[len("cwgen_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "cwgen_*.npz")))
               if n != "tables" and not n.startswith("chain_"))
SETTINGS = ("mode", "speed", "weight", "reverse", "rx_delay", "sidetone", "capacity")
PER_BLOCK = ("cw_state", "key_timer", "sm_tbl_ptr", "port_state", "acc")
WINDOW = 256
ECHO_CAPACITY = 64
CHAIN_CASES = sorted(os.path.basename(p)[len("cwgen_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "cwgen_chain_*.npz")))
_cache = {}


def load_chain_case(name):
    """A recording of the CW transmit chain at 32-frame calls: the keyer's settings, cw_lsb, the text
    put before the first call, a key byte and a flag byte per call, a crc32 per call of the int32 I/Q
    frames and of a_buffer[0], three raw windows of each, consumed and echo.  args: the harness'
    arguments (mode, iqmode, gains, `tune` as "first call:calls:1")."""
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, f"cwgen_{name}.npz")) as z:
            g = {k: z[k] for k in z.files}
        g["name"] = name
        g["args"] = json.loads(str(g["args"]))
        g["text"], g["echo"] = bytes(g["text"]), bytes(g["echo"])
        for k in SETTINGS + ("cw_lsb", "frames", "consumed"):
            g[k] = int(g[k])
        calls = g["frames"] // 32
        assert len(g["keys"]) == len(g["flags"]) == len(g["iq_crc"]) == len(g["a0_crc"]) == calls
        assert g["iq_win"].shape == (3, WINDOW, 2) and g["a0_win"].shape == (3, WINDOW)
        t = g["args"].pop("tune", None)
        g["tune"] = tuple(int(x) for x in t.split(":")[:2]) if t else None      # (first call, calls)
        _cache[name] = g
    return _cache[name]


def check_chain(g, iq, a0):
    """iq int32 [frames][2], a0 float32 [frames] of one channel against the recording, bit for bit"""
    n = g["frames"]
    assert iq.shape == (n, 2) and a0.shape == (n,)
    for what, got, crc, win in (("iq", np.ascontiguousarray(iq), g["iq_crc"], g["iq_win"]), ("a0", np.ascontiguousarray(a0), g["a0_crc"], g["a0_win"])):
        mine = np.array([zlib.crc32(got[k:k + 32].tobytes()) for k in range(0, n, 32)], np.uint32)
        bad = np.flatnonzero(mine != crc)
        assert len(bad) == 0, f"{g['name']}: {what} of call {bad[0]} differs ({len(bad)} of {len(crc)} calls)"
        for at, w in zip(g["window_at"], win):
            assert np.array_equal(got[at:at + WINDOW].view(np.uint32), w.view(np.uint32)), f"{g['name']}: {what} window at {at}"


def load_case(name):
    """The fixture as a dict.  ops as [["put", bytes], ["speed", wpm, weight], ["blk", lines, count]];
    `keys` uint8 [B] the key lines of every block; `events` [(block, op)] the puts and speed changes
    with the block they come before."""
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, f"cwgen_{name}.npz")) as z:
            g = {k: z[k] for k in z.files}
        g["name"] = name
        g["ops"] = [[op[0], bytes.fromhex(op[1])] if op[0] == "put" else op for op in json.loads(str(g["ops"]))]
        for k in SETTINGS + ("consumed",):
            g[k] = int(g[k])
        g["echo"] = bytes(g["echo"])
        keys, events = [], []
        for op in g["ops"]:
            if op[0] == "blk":
                keys += [op[1]] * op[2]
            else:
                events.append((len(keys), op))
        g["keys"] = np.array(keys, np.uint8)
        g["events"] = events
        g["blocks"] = B = len(keys)
        assert all(len(g[k]) == B for k in PER_BLOCK + ("flags", "i_crc", "q_crc"))
        assert g["i_win"].shape == g["q_win"].shape == (3, WINDOW) and len(g["accepted"]) == sum(op[0] == "put" for op in g["ops"])
        assert len(g["echo"]) <= ECHO_CAPACITY
        for v in g.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = g
    return _cache[name]


def make(g, channels=1, host=True, stream=None):
    """a generator with the fixture's settings"""
    return cwgen.CwGenerator(channels, g["mode"], g["speed"], g["weight"], g["reverse"], g["rx_delay"], g["sidetone"],
                             capacity=g["capacity"], echo_capacity=ECHO_CAPACITY, host=host, stream=stream)


def cuts(g, chunk):
    """block indices at which a run of the case is cut into calls: every event, and every `chunk`
    blocks (None: only the events)"""
    at = {0, g["blocks"]} | {b for b, _ in g["events"]}
    if chunk:
        at |= set(range(0, g["blocks"], chunk))
    return sorted(at)


def run_host(g, chunk=None, channels=1, at=0, each_block=False):
    """The case on channel `at` of a host generator, the other channels idle.  Returns i, q float32
    [32 B], flags uint8 [B], accepted, consumed, echo, and with each_block (32-sample calls) the
    keyer's words after every block as a dict of uint32 [B]."""
    gen = make(g, channels)
    B = g["blocks"]
    i, q = np.zeros(32 * B, np.float32), np.zeros(32 * B, np.float32)
    flags, accepted = np.zeros(B, np.uint8), []
    words = {k: np.zeros(B, np.uint32) for k in cwgen.WORDS} if each_block else None
    edges = cuts(g, 1 if each_block else chunk)
    events = dict()
    for b, op in g["events"]:
        events.setdefault(b, []).append(op)
    for b0, b1 in zip(edges[:-1], edges[1:]):
        for op in events.get(b0, []):
            if op[0] == "put":
                accepted.append(int(gen.put_text([op[1] if c == at else b"" for c in range(channels)])[at]))
            else:
                gen.set_speed(op[1], op[2])
        keys = np.zeros((channels, b1 - b0), np.uint8)
        keys[at] = g["keys"][b0:b1]
        bi, bq = np.full((channels, 32 * (b1 - b0) + 5), 7.0, np.float32), np.full((channels, 32 * (b1 - b0) + 5), 7.0, np.float32)
        gen.process(keys, bi, bq, 32 * (b1 - b0))
        assert (bi[:, -5:] == 7.0).all() and (bq[:, -5:] == 7.0).all()          # n < stride: the tail stays
        i[32 * b0:32 * b1], q[32 * b0:32 * b1] = bi[at, :-5], bq[at, :-5]
        flags[b0:b1] = gen.flags()[at]
        if each_block:
            for k, v in gen.peek().items():
                words[k][b0] = v[at]
    out = dict(i=i, q=q, flags=flags, accepted=accepted, consumed=int(gen.consumed()[at]), echo=gen.echo()[at], state=int(gen.state()[at]), words=words)
    gen.close()
    return out


def block_crc(x):
    x = np.ascontiguousarray(x)
    return np.array([zlib.crc32(x[k:k + 32].tobytes()) for k in range(0, len(x), 32)], np.uint32)


def check_samples(g, i, q, blocks=None):
    """one channel's I and Q from block 0 against the recording: every block's crc32 and the windows, bit for bit"""
    B = g["blocks"] if blocks is None else blocks
    for what, got, crc, win in (("i", i, g["i_crc"], g["i_win"]), ("q", q, g["q_crc"], g["q_win"])):
        assert len(got) >= 32 * B
        bad = np.flatnonzero(block_crc(got[:32 * B]) != crc[:B])
        assert len(bad) == 0, f"{g['name']}: {what} of block {bad[0]} differs ({len(bad)} of {B} blocks)"
        for at, w in zip(g["window_at"], win):
            if at + WINDOW <= 32 * B:
                assert np.array_equal(np.ascontiguousarray(got[at:at + WINDOW]).view(np.uint32), w.view(np.uint32)), f"{g['name']}: {what} window at {at}"


def check_run(g, r):
    """a whole run of run_host against the recording"""
    check_samples(g, r["i"], r["q"])
    assert np.array_equal(r["flags"], g["flags"]), f"{g['name']}: flags differ first in block {np.flatnonzero(r['flags'] != g['flags'])[:1]}"
    assert r["accepted"] == g["accepted"].tolist(), g["name"]
    assert r["consumed"] == g["consumed"] and r["echo"] == g["echo"], (g["name"], r["consumed"], r["echo"])
    assert r["state"] == int(g["key_timer"][-1] if g["mode"] == cwgen.STRAIGHT else g["cw_state"][-1])
    if r["words"] is not None:
        for k in PER_BLOCK:
            got, want = r["words"][k], g[k].astype(np.uint32)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, f"{g['name']}: {k} differs first after block {bad[0]}: {got[bad[0]]} for {want[bad[0]]}"
