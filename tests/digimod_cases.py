"""Loader and runner of the modulator fixtures (tests/golden/digimod_*.npz, recorded from the
reference firmware by tools/digimod/make_digimod_golden.py)."""
import glob
import json
import os
import zlib

import numpy as np

from uhsdr_amd import digimod

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_ALL = sorted(os.path.basename(p)[len("digimod_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "digimod_*.npz")))
CASES = [n for n in _ALL if not n.startswith(("loop_", "chain_"))]
LOOP_CASES = [n for n in _ALL if n.startswith("loop_")]      # modulator into decoder
CHAIN_CASES = [n for n in _ALL if n.startswith("chain_")]    # TxProcessor_Run in DIGI mode


def load_chain_case(name):
    """A recording of the DIGI transmit chain at 32-frame calls: a crc32 per call of the int32 I/Q
    frames and of a_buffer[0], three raw windows of each, the modulator's outputs at the end."""
    with np.load(os.path.join(GOLDEN, f"digimod_{name}.npz")) as z:
        g = {k: z[k] for k in z.files}
    g["name"] = name
    g["kind"] = str(g["kind"])
    g["args"] = json.loads(str(g["args"]))
    g["text"] = bytes(g["text"])
    for k in ("shift_idx", "speed_idx", "stopbits_idx", "capacity", "frames", "consumed", "state"):
        g[k] = int(g[k])
    assert len(g["iq_crc"]) == len(g["a0_crc"]) == g["frames"] // 32
    assert g["iq_win"].shape == (3, WINDOW, 2) and g["a0_win"].shape == (3, WINDOW)
    return g


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
BLOCK, WINDOW = 1024, 256
_cache = {}


def load_loop_case(name):
    """A loopback recording.  `chars` is what the reference decoder printed behind `lead` samples of
    silence; whether that holds the message is recorded in `verbatim`, and is not asserted here."""
    with np.load(os.path.join(GOLDEN, f"digimod_{name}.npz")) as z:
        g = {k: z[k] for k in z.files}
    g["name"] = name
    g["kind"] = str(g["kind"])
    g["ops"] = [[op[0], bytes.fromhex(op[1])] if op[0] == "put" else op for op in json.loads(str(g["ops"]))]
    for k in ("shift_idx", "speed_idx", "stopbits_idx", "capacity", "lead"):
        g[k] = int(g[k])
    assert g["lead"] in g["leads"] and bool(g["verbatim"]) == (bytes(g["message"]) in bytes(g["chars"]))
    return g


def load_case(name):
    """the fixture as a dict; ops as [["put", bytes], ["gen", n], ["start"]]"""
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, f"digimod_{name}.npz")) as z:
            g = {k: z[k] for k in z.files}
        g["name"] = name
        g["kind"] = str(g["kind"])
        g["ops"] = [[op[0], bytes.fromhex(op[1])] if op[0] == "put" else op for op in json.loads(str(g["ops"]))]
        for k in ("shift_idx", "speed_idx", "stopbits_idx", "capacity", "total"):
            g[k] = int(g[k])
        gens = [op[1] for op in g["ops"] if op[0] == "gen"]
        assert sum(gens) == g["total"] and len(gens) == len(g["consumed"]) == len(g["txoff_at"]) == len(g["state"])
        assert len(g["accepted"]) == sum(op[0] == "put" for op in g["ops"])
        if g["total"] <= 65536:
            assert g["samples"].dtype == np.int16 and len(g["samples"]) == g["total"]
        else:
            assert len(g["block_crc"]) == -(-g["total"] // BLOCK) and g["windows"].shape == (3, WINDOW)
        _cache[name] = g
    return _cache[name]


def make(g, channels=1, host=True, stream=None):
    """a modulator with the fixture's parameters"""
    if g["kind"] == "rtty":
        return digimod.RttyModulator(channels, g["shift_idx"], g["speed_idx"], g["stopbits_idx"], capacity=g["capacity"], host=host, stream=stream)
    return digimod.PskModulator(channels, g["speed_idx"], capacity=g["capacity"], host=host, stream=stream)


def start(mod):
    mod.start_tx() if isinstance(mod, digimod.RttyModulator) else mod.prepare_tx()


def run_ops(mod, ops, chunk=None, carries=None, new_audio=None):
    """The ops on every channel of `mod` for which carries(c) holds (default: all; the others get no
    text), generating at most `chunk` samples per call.  Returns samples int16 [C][total], the
    accepted counts of every put [puts][C], and consumed / txoff_at / state after every gen
    [gens][C].  new_audio(stride) makes the buffer a call writes (default: a host array)."""
    C = mod.channels
    on = [carries is None or bool(carries(c)) for c in range(C)]
    out, accepted, after = [], [], []
    for op in ops:
        if op[0] == "put":
            accepted.append(mod.put_text([op[1] if on[c] else b"" for c in range(C)]))
        elif op[0] == "start":
            start(mod)
        else:
            n = op[1]
            step = n if chunk is None else chunk
            for b in range(0, n, step):
                m = min(step, n - b)
                if new_audio is None:
                    buf = np.full((C, m + 3), 0x5a5a, np.int16)         # n < stride: the tail stays
                    mod.process(buf, m)
                    assert (buf[:, m:] == 0x5a5a).all()
                    out.append(buf[:, :m].copy())
                else:
                    buf = new_audio(m + 3)
                    mod.process(buf, m)
                    out.append(buf)
            after.append((mod.consumed(), mod.txoff_at(), mod.state()))
    if new_audio is not None:
        mod.synchronize()
        tails = [np.asarray(b.cpu().numpy()) for b in out]
        assert all((t[:, -3:] == 0x5a5a).all() for t in tails)
        out = [t[:, :-3] for t in tails]
    samples = np.concatenate(out, axis=1) if out else np.zeros((C, 0), np.int16)
    return (samples, np.array(accepted, np.int32).reshape(-1, C),
            tuple(np.array([a[k] for a in after]).reshape(-1, C) for k in range(3)))


def check_samples(g, row, upto=None):
    """row: one channel's int16 samples from sample 0; compares the first `upto` (default: all the
    fixture has) with the recording: the samples whole, or every complete block's crc32 and the windows"""
    n = g["total"] if upto is None else min(upto, g["total"])
    assert len(row) >= n
    if "samples" in g:
        assert np.array_equal(row[:n], g["samples"][:n]), g["name"]
        return
    blocks = n // BLOCK if n < g["total"] else len(g["block_crc"])
    got = np.array([zlib.crc32(np.ascontiguousarray(row[k * BLOCK:min((k + 1) * BLOCK, n)]).tobytes()) for k in range(blocks)], np.uint32)
    bad = np.flatnonzero(got != g["block_crc"][:blocks])
    assert len(bad) == 0, f"{g['name']}: block {bad[0]} of {blocks} differs"
    for at, w in zip(g["window_at"], g["windows"]):
        if at + WINDOW <= n:
            assert np.array_equal(row[at:at + WINDOW], w), f"{g['name']}: window at {at}"


def check_outputs(g, accepted, after, c=0):
    """the put counts and the outputs after every gen of channel c against the recording"""
    consumed, txoff_at, state = after
    assert np.array_equal(accepted[:, c], g["accepted"]), g["name"]
    assert np.array_equal(consumed[:, c], g["consumed"]), g["name"]
    assert np.array_equal(txoff_at[:, c], g["txoff_at"]), g["name"]
    assert np.array_equal(state[:, c], g["state"]), g["name"]
