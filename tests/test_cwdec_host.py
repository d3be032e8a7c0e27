"""CW decoder back end on the CPU (uhsdr_cwdec_process_host: the step function the cw_decode kernel
runs) against what the reference firmware's decoder printed (tests/golden/cwtext_*.npz, recorded
by tools/cwtext/make_cwtext_golden.py).  Everything is exact: bytes, their block, the WPM byte."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import uhsdr_amd as U
from uhsdr_amd import cwdec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("cwtext_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "cwtext_*.npz"))
               if not p.endswith("chartable.npz"))


def load_case(name):
    z = np.load(os.path.join(GOLDEN, f"cwtext_{name}.npz"))
    return {k: z[k] for k in z.files}


def test_fixture_set_covers_the_decoder():
    assert len(CASES) >= 12
    texts = {n: bytes(load_case(n)["chars"]) for n in CASES}
    assert any(b"#" in t for t in texts.values())
    assert {int(load_case(n)["spikecancel"]) for n in CASES} == {0, 1, 2}
    assert {int(load_case(n)["blocksize"]) for n in CASES} >= {60, 88, 128}


@pytest.mark.parametrize("name", CASES)
def test_one_piece(name):
    g = load_case(name)
    state = np.ascontiguousarray(g["state"][None, :])
    for cap in (8, 64):
        d = cwdec.CwDecoder(1, int(g["blocksize"]), int(g["spikecancel"]), cap, host=True)
        d.process(state)
        text, total, wpm = d.read()
        n = len(g["chars"])
        assert int(total[0]) == n
        k = np.arange(max(0, n - cap), n)
        assert bytes(text[0, k % cap]) == bytes(g["chars"][k])
        assert int(wpm[0]) == int(g["speed"][-1])
        d.close()
    # the whole text and the speed after every block: a large ring, one block per call
    d = cwdec.CwDecoder(1, int(g["blocksize"]), int(g["spikecancel"]), 4096, host=True)
    blocks = min(len(g["state"]), 6000)
    speed = np.empty(blocks, np.uint8)
    for b in range(blocks):
        d.process(state[:, b:b + 1].copy())
        speed[b] = d.outputs.read()[2][0]
    assert np.array_equal(speed, g["speed"][:blocks])
    d.process(np.ascontiguousarray(state[:, blocks:]))
    text, total, wpm = d.read()
    assert bytes(text[0, :int(total[0])]) == bytes(g["chars"])
    assert int(wpm[0]) == int(g["speed"][-1])
    d.close()


@pytest.mark.parametrize("per_call", [1, 7, 97])
@pytest.mark.parametrize("name", CASES)
def test_in_calls(name, per_call):
    g = load_case(name)
    state = g["state"]
    blocks = len(state) if per_call > 1 else min(len(state), 5000)
    d = cwdec.CwDecoder(1, int(g["blocksize"]), int(g["spikecancel"]), 16, host=True)
    for b in range(0, blocks, per_call):
        chunk = np.ascontiguousarray(state[None, b:min(b + per_call, blocks)])
        d.process(chunk)
        done = b + chunk.shape[1]
        _, total, wpm = d.outputs.read()
        assert int(total[0]) == int(np.count_nonzero(g["char_block"] < done)), (name, done)
        assert int(wpm[0]) == int(g["speed"][done - 1]), (name, done)
    d.close()


def test_channels_are_independent():
    """different cases side by side in one host handle, rows padded to one stride"""
    gs = [load_case(n) for n in CASES if int(load_case(n)["blocksize"]) == 88 and int(load_case(n)["spikecancel"]) == 0]
    assert len(gs) >= 4
    blocks = min(len(g["state"]) for g in gs)
    state = np.stack([g["state"][:blocks] for g in gs])
    d = cwdec.CwDecoder(len(gs), 88, 0, 4096, host=True)
    d.process(np.ascontiguousarray(state))
    text, total, wpm = d.read()
    for c, g in enumerate(gs):
        n = int(np.count_nonzero(g["char_block"] < blocks))
        assert int(total[c]) == n and bytes(text[c, :n]) == bytes(g["chars"][:n])
        assert int(wpm[c]) == int(g["speed"][blocks - 1])
    assert b"".join(d.outputs.new_text()) == b"".join(bytes(g["chars"][:np.count_nonzero(g["char_block"] < blocks)]) for g in gs)
    assert d.outputs.new_text() == [b""] * len(gs)
    d.close()


def test_character_table():
    z = np.load(os.path.join(GOLDEN, "cwtext_chartable.npz"))
    assert len(z["code"]) == 1023
    got = np.array([cwdec.char_id(int(c)) for c in z["code"]], np.uint8)
    assert np.array_equal(got, z["char"])


def test_argument_errors():
    lib = U.load()
    h = C.c_void_p()
    for args in ((0, 88, 0, 64), (4, 7, 0, 64), (4, 129, 0, 64), (4, 88, 3, 64), (4, 88, -1, 64), (4, 88, 0, 7)):
        assert lib.uhsdr_cwdec_create_host(*args, C.byref(h)) == -1, args
        assert lib.uhsdr_cwdec_create(*args, None, C.byref(h)) == -1, args      # refused before any device call
    assert b"text_capacity" in lib.uhsdr_last_error()
    assert lib.uhsdr_cwdec_create_host(4, 88, 0, 64, None) == -1
    assert lib.uhsdr_cwdec_create_host(4, 8, 2, 8, C.byref(h)) == 0
    st = np.zeros((4, 16), np.uint8)
    assert lib.uhsdr_cwdec_process_host(h, None, 4, 16) == -1
    assert lib.uhsdr_cwdec_process_host(h, st.ctypes.data_as(C.c_void_p), 17, 16) == -2
    assert lib.uhsdr_cwdec_process_host(h, st.ctypes.data_as(C.c_void_p), -1, 16) == -2
    assert lib.uhsdr_cwdec_process(h, st.ctypes.data_as(C.c_void_p), 4, 16) == -1          # a host handle
    assert lib.uhsdr_cwdec_process_host(h, st.ctypes.data_as(C.c_void_p), 16, 16) == 0
    assert lib.uhsdr_cwdec_destroy(h) == 0
    assert lib.uhsdr_cwdec_process_host(None, st.ctypes.data_as(C.c_void_p), 4, 16) == -1
    assert lib.uhsdr_rx_set_cw_text(None, 1, 0, 64) == -1
    assert lib.uhsdr_rx_cw_text_outputs(None, None, None, None) == -1


def test_arbitrary_input_stays_in_bounds():
    """pseudo-random run-length streams, including one that starts on a mark (a zero-length first
    state) and one-block runs: the decoder terminates and its counters stay inside the state"""
    rng = np.random.default_rng(7)
    rows = []
    for c in range(16):
        runs = rng.integers(1, 3 + 6 * (c % 5), size=4096)
        row = np.repeat((np.arange(len(runs)) + c) % 2, runs)[:4096].astype(np.uint8)
        rows.append(row)
    state = np.ascontiguousarray(np.stack(rows))
    for bs, sc in ((8, 0), (72, 2), (128, 1)):
        d = cwdec.CwDecoder(16, bs, sc, 8, host=True)
        d.process(state)
        e = cwdec.CwDecoder(16, bs, sc, 8, host=True)
        for b in range(0, 4096, 512):
            e.process(np.ascontiguousarray(state[:, b:b + 512]))
        for x, y in zip(d.read(), e.read()):
            assert np.array_equal(x, y)
        d.close()
        e.close()
