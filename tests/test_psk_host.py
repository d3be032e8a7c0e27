"""BPSK decoder on the CPU (uhsdr_psk_process_host: the step functions the psk_decode kernel runs)
against what the reference firmware's decoder printed (tests/golden/psk_*.npz, recorded by
tools/psk/make_psk_golden.py).  Everything is exact: the bytes and the sample that emitted each."""
import ctypes as C

import numpy as np
import pytest

import uhsdr_amd as U
from uhsdr_amd import psk, synth

from psk_cases import CASES, CHAIN_CASES, EXPECT, load_case, load_chain_case


def test_fixture_set_covers_the_decoder():
    assert set(CASES) == set(EXPECT)
    gs = {n: load_case(n) for n in CASES}                  # (the loader asserts what each recording shows)
    assert {gs[n]["speed"] for n in ("clean31", "clean63", "clean125")} == {0, 1, 2}
    table = bytes(gs["chartable125"]["chars"])
    assert gs["chartable125"]["sent"] == bytes(range(256)) and all(bytes([b]) in table for b in range(256))
    assert bytes(gs["tiny"]["chars"]) == bytes(gs["clean125"]["chars"])       # the denormal product is not flushed
    assert b"*" in bytes(gs["idle60"]["chars"])[:3]                     # rx_word wrapped: no code matches
    assert bytes(gs["noisy_b"]["chars"]) != bytes(gs["noisy_a"]["chars"])
    assert len({bytes(gs[n]["chars"]) for n in ("df0p5", "df1", "df2")}) == 3
    assert len({tuple(gs[f"offsets63_{k}"]["char_sample"]) for k in range(8)}) > 1


def test_varicode_alphabet():
    codes = synth.varicode_table()
    assert len(codes) == 256 and len(set(codes)) == 256 and max(codes) < 4096
    for c in codes:
        b = bin(c)[2:]
        assert b[0] == "1" and b[-1] == "1" and "00" not in b
    assert codes[ord(" ")] == 1 and codes[ord("e")] == 3 and codes[ord("t")] == 5
    assert synth.varicode_bits("e", preamble=2, postamble=1).tolist() == [0, 0, 1, 1, 0, 0, 0]


def run_in_calls(g, per_call, cap=4096):
    """the decoder fed `per_call` samples at a time: text, total, and the total after every call"""
    lib = U.load()
    audio = g["audio"]
    d = psk.PskDecoder(1, g["speed"], capacity=cap, host=True)
    total = C.cast(d.outputs.ptr[1], C.POINTER(C.c_uint32))
    p = audio.ctypes.data
    after = []
    for b in range(0, len(audio), per_call):
        m = min(per_call, len(audio) - b)
        assert lib.uhsdr_psk_process_host(d.handle, C.c_void_p(p + 4 * b), m, m) == 0
        after.append(total[0])
    text, tot = d.read()
    d.close()
    return text, tot, np.array(after, np.int64)


@pytest.mark.parametrize("name", CASES)
def test_one_piece(name):
    g = load_case(name)
    audio = np.ascontiguousarray(g["audio"][None, :])
    n = len(g["chars"])
    for cap in (8, 4096):
        d = psk.PskDecoder(1, g["speed"], capacity=cap, host=True)
        d.process(audio)
        text, total = d.read()
        assert int(total[0]) == n
        k = np.arange(max(0, n - cap), n)
        assert bytes(text[0, k % cap]) == bytes(g["chars"][k])
        sym = d.symbol().copy()
        d.reset()                                   # reset reproduces the run
        assert d.read()[1][0] == 0 and d.symbol().view(np.uint32)[0] == 0
        d.process(audio)
        text2, total2 = d.read()
        assert np.array_equal(total2, total) and np.array_equal(text2, text)
        assert np.array_equal(d.symbol().view(np.uint32), sym.view(np.uint32))
        d.close()


@pytest.mark.parametrize("per_call", [8, 23, 25, 333, 1000])
@pytest.mark.parametrize("name", CASES)
def test_in_calls(name, per_call):
    """the same bytes, each present after the call that holds its sample and not before"""
    g = load_case(name)
    samples = len(g["audio"])
    text, tot, after = run_in_calls(g, per_call)
    emitted = np.zeros(samples + 1, np.int64)           # characters complete after sample i
    np.add.at(emitted, g["char_sample"], 1)
    emitted = np.cumsum(emitted)
    ends = np.minimum(np.arange(per_call, samples + per_call, per_call), samples) - 1
    assert np.array_equal(after, emitted[ends]), name
    assert int(tot[0]) == len(g["chars"]) and bytes(text[0, :int(tot[0])]) == bytes(g["chars"])


def test_channels_are_independent():
    """different cases of one speed side by side in one host handle, rows padded to one stride"""
    gs = [load_case(n) for n in CASES if load_case(n)["speed"] == 2 and n != "chartable125"]
    assert len(gs) >= 8
    stride = max(len(g["audio"]) for g in gs) + 5
    n = min(len(g["audio"]) for g in gs)
    rows = np.zeros((len(gs), stride), np.float32)
    for c, g in enumerate(gs):
        rows[c, :len(g["audio"])] = g["audio"]
    d = psk.PskDecoder(len(gs), 2, capacity=4096, host=True)
    d.process(rows, n)
    text, total = d.read()
    want = [bytes(g["chars"][g["char_sample"] < n]) for g in gs]
    for c, w in enumerate(want):
        assert int(total[c]) == len(w) and bytes(text[c, :len(w)]) == w
    assert d.outputs.new_text() == want
    assert d.outputs.new_text() == [b""] * len(gs)
    # a row alone gives the symbol it gave among the others
    sym = d.symbol()
    for c in (0, len(gs) - 1):
        e = psk.PskDecoder(1, 2, capacity=8, host=True)
        e.process(np.ascontiguousarray(rows[c:c + 1]), n)
        assert e.symbol().view(np.uint32)[0] == sym.view(np.uint32)[c]
        e.close()
    d.close()


def test_symbol_is_finite_on_arbitrary_input():
    """finite input of any scale, zeros and denormals: the symbol output stays finite and chunking
    does not matter; infinities and NaN terminate as well"""
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((10, 6000)) * 10.0 ** rng.integers(-44, 30, size=(10, 1))).astype(np.float32)
    x[1, 2000:4000] = 0.0
    x[2] = 1e30
    x[3] = np.float32(1e-45)
    for speed in range(3):
        d = psk.PskDecoder(10, speed, capacity=8, host=True)
        d.process(x)
        e = psk.PskDecoder(10, speed, capacity=8, host=True)
        for b in range(0, 6000, 500):
            e.process(np.ascontiguousarray(x[:, b:b + 500]))
        assert np.isfinite(d.symbol()).all() and np.count_nonzero(d.symbol()) >= 8
        for u, v in zip(d.read() + (d.symbol().view(np.uint32),), e.read() + (e.symbol().view(np.uint32),)):
            assert np.array_equal(u, v)
        d.close()
        e.close()
    x[4, 100] = np.nan
    x[5, 200] = np.inf
    x[6, 300:310] = -np.inf
    x[7, :] = 3.0e38
    d = psk.PskDecoder(10, 2, capacity=8, host=True)
    d.process(x)
    assert np.isfinite(d.symbol()[:4]).all() and not np.isfinite(d.symbol()[4:8]).any()
    d.close()


def test_argument_errors():
    lib = U.load()
    h = C.c_void_p()
    for args in ((0, 0, 64), (4, -1, 64), (4, 3, 64), (4, 0, 7)):
        assert lib.uhsdr_psk_create_host(*args, C.byref(h)) == -1, args
        assert lib.uhsdr_psk_create(*args, None, C.byref(h)) == -1, args      # refused before any device call
    assert b"text_capacity" in lib.uhsdr_last_error()
    assert lib.uhsdr_psk_create_host(4, 3, 64, C.byref(h)) == -1 and b"speed_idx" in lib.uhsdr_last_error()
    assert lib.uhsdr_psk_create_host(4, 0, 64, None) == -1
    assert lib.uhsdr_psk_create_host(4, 2, 8, C.byref(h)) == 0
    x = np.zeros((4, 16), np.float32)
    assert lib.uhsdr_psk_process_host(h, None, 4, 16) == -1
    assert lib.uhsdr_psk_process_host(h, x.ctypes.data_as(C.c_void_p), 17, 16) == -2
    assert lib.uhsdr_psk_process_host(h, x.ctypes.data_as(C.c_void_p), -1, 16) == -2
    assert lib.uhsdr_psk_process(h, x.ctypes.data_as(C.c_void_p), 4, 16) == -1          # a host handle
    assert lib.uhsdr_psk_set_stream(h, None) == -1
    assert lib.uhsdr_psk_process_host(h, x.ctypes.data_as(C.c_void_p), 16, 16) == 0
    assert lib.uhsdr_psk_process_host(h, x.ctypes.data_as(C.c_void_p), 0, 16) == 0
    assert lib.uhsdr_psk_destroy(h) == 0
    assert lib.uhsdr_psk_process_host(None, x.ctypes.data_as(C.c_void_p), 4, 16) == -1
    assert lib.uhsdr_psk_outputs(None, None, None, None) == -1
    assert lib.uhsdr_psk_reset(None) == -1
    # the receive chain's entry points (no device call on a null handle)
    assert lib.uhsdr_rx_set_psk_text(None, 1, 0, 64) == -1
    assert lib.uhsdr_rx_psk_text_outputs(None, None, None, None) == -1
    assert lib.uhsdr_abi_version() == 9


def test_chain_fixtures_regenerate():
    """the two recordings through the receive chain: inputs regenerate to the recorded crc32, the
    reference printed the message verbatim, one tap crc32 per 32-frame call"""
    assert CHAIN_CASES == ["chain_p48_125", "chain_p48_31"]
    gs = [load_chain_case(n) for n in CHAIN_CASES]
    assert [g["speed"] for g in gs] == [2, 0]
    for g in gs:
        assert int(g["path"]) == 48 and len(g["tap_crc"]) == len(g["iq"]) // 32 and len(g["tap_head"]) == 256
        assert str(g["message"]).encode() in bytes(g["chars"])


def test_psk_iq_carries_the_text():
    """synth.psk_iq mixed down from its carrier and sampled at 12 ksps decodes to the message on
    every channel, generated in one piece or in chunks (absolute sample index)"""
    msg = "de UHSDR 73 "
    n = 48000 * 5
    whole = synth.psk_iq(np.arange(3), 0, n, msg, baud=125.0, noise_sigma=0.0, lead=4800)
    parts = np.concatenate([synth.psk_iq(np.arange(3), s, min(100001, n - s), msg, baud=125.0, noise_sigma=0.0, lead=4800)
                            for s in range(0, n, 100001)], axis=1)
    assert np.array_equal(whole, parts)
    z = (whole[..., 0] >> 16) + 1j * (whole[..., 1] >> 16)
    audio = (z * np.exp(-2j * np.pi * 12000.0 / 48000.0 * np.arange(n))).real[:, ::4]
    d = psk.PskDecoder(3, psk.SPEED_125, capacity=256, host=True)
    d.process(np.ascontiguousarray(audio, dtype=np.float32))
    for t in d.new_text():
        assert msg.encode() in t, t
    d.close()
