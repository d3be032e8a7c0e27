"""RTTY and BPSK modulators on the CPU (uhsdr_rttymod_process_host / uhsdr_pskmod_process_host: the
step functions the rttymod_gen / pskmod_gen kernels run) against what the reference firmware's
Rtty_Modulator_GenSample / Psk_Modulator_GenSample returned (tests/golden/digimod_*.npz, recorded by
tools/digimod/make_digimod_golden.py).  Everything is exact: every int16, the characters taken, the
sample of the TX-off request and the BPSK state."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

import uhsdr_amd as U
from uhsdr_amd import digimod, psk, rtty

from digimod_cases import (CASES, CHAIN_CASES, LOOP_CASES, check_outputs, check_samples, load_case, load_chain_case, load_loop_case,
                           make, run_ops)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_set_covers_the_modulators():
    gs = {n: load_case(n) for n in CASES}
    rs = [g for g in gs.values() if g["kind"] == "rtty"]
    ps = [g for g in gs.values() if g["kind"] == "psk"]
    assert {g["stopbits_idx"] for g in rs if (g["shift_idx"], g["speed_idx"]) == (1, 0)} == {0, 1, 2}
    assert {g["speed_idx"] for g in rs} == {0, 1} and {0, 5} <= {g["shift_idx"] for g in rs}
    assert {g["speed_idx"] for g in ps} == {0, 1, 2}
    assert gs["rtty_idle"]["consumed"][-1] == 0 and gs["psk_31_idle"]["consumed"][-1] == 0
    assert gs["rtty_bytes"]["ops"][0][1] == bytes(range(128)) and gs["rtty_bytes"]["consumed"][-1] == 128
    assert gs["psk_125_ascii"]["ops"][0][1] == bytes(range(128)) and gs["psk_125_ascii"]["consumed"][-1] == 128
    assert min(gs["psk_125_high"]["ops"][0][1]) >= 0x80 and gs["psk_125_high"]["consumed"][-1] == 27
    # EOT: RTTY requests TX-off and goes on with the text; BPSK turns OFF after the postamble
    assert gs["rtty_eot"]["txoff_at"][-1] != digimod.NO_TXOFF and gs["rtty_eot"]["consumed"][-1] == 6
    assert gs["psk_63_eot"]["state"][-1] == digimod.PSK_OFF and gs["psk_63_eot"]["txoff_at"][-1] != digimod.NO_TXOFF
    assert gs["psk_125_eot"]["state"].tolist() == [digimod.PSK_OFF, digimod.PSK_ACTIVE]         # prepare_tx after OFF
    assert gs["psk_31_idle"]["state"][-1] == digimod.PSK_ACTIVE
    # a queue of 8 holds 7
    assert gs["rtty_late_cap8"]["accepted"].tolist() == [7, 5] and gs["psk_31_cap8"]["accepted"].tolist() == [7, 7]
    assert any(op == ["start"] for op in gs["rtty_restart"]["ops"])


def test_fixtures_regenerate_their_inputs():
    """the recorder's case list gives the parameters and ops every committed fixture holds"""
    sys.path.insert(0, os.path.join(ROOT, "tools", "digimod"))
    try:
        import make_digimod_golden as maker
    finally:
        sys.path.pop(0)
    made = {c["name"]: c for c in maker.cases()}
    assert sorted(made) == CASES
    for name, c in made.items():
        g = load_case(name)
        assert [g[k] for k in ("kind", "shift_idx", "speed_idx", "stopbits_idx", "capacity")] == \
               [c[k] for k in ("kind", "shift_idx", "speed_idx", "stopbits_idx", "capacity")]
        assert [[op[0], op[1].hex()] if op[0] == "put" else op for op in g["ops"]] == c["ops"]
    chains = {c["name"]: c for c in maker.chain_cases()}
    assert sorted(chains) == CHAIN_CASES
    for name, c in chains.items():
        g = load_chain_case(name)
        m = c["mod"]
        assert g["args"] == c["args"] and g["text"].hex() == m["ops"][0][1] and g["frames"] == maker.CHAIN_FRAMES
        assert [g[k] for k in ("kind", "shift_idx", "speed_idx", "stopbits_idx", "capacity")] == \
               [m[k] for k in ("kind", "shift_idx", "speed_idx", "stopbits_idx", "capacity")]
    loops = {c["name"]: c for c in maker.loop_cases()}
    assert sorted(loops) == LOOP_CASES
    for name, c in loops.items():
        g = load_loop_case(name)
        assert bytes(g["message"]) == c["message"] and g["leads"].tolist() == c["leads"]
        assert [[op[0], op[1].hex()] if op[0] == "put" else op for op in g["ops"]] == c["mod"]["ops"]


@pytest.mark.parametrize("name", CASES)
def test_one_piece(name):
    g = load_case(name)
    mod = make(g)
    samples, accepted, after = run_ops(mod, g["ops"])
    check_samples(g, samples[0])
    check_outputs(g, accepted, after)
    mod.reset()                                     # reset reproduces the run
    assert mod.consumed()[0] == 0 and mod.txoff_at()[0] == digimod.NO_TXOFF
    again, accepted2, after2 = run_ops(mod, g["ops"])
    assert np.array_equal(again, samples) and np.array_equal(accepted2, accepted)
    assert all(np.array_equal(u, v) for u, v in zip(after, after2))
    mod.close()


@pytest.mark.parametrize("chunk", [1, 31, 33, 1000])
@pytest.mark.parametrize("name", CASES)
def test_in_calls(name, chunk):
    g = load_case(name)
    mod = make(g)
    if chunk == 1:
        # one call per sample, without the runner's buffers: the ops by hand
        lib, out, accepted, after = U.load(), [], [], []
        fn = lib.uhsdr_rttymod_process_host if g["kind"] == "rtty" else lib.uhsdr_pskmod_process_host
        for op in g["ops"]:
            if op[0] == "gen":
                row = np.zeros(op[1], np.int16)
                h, status = mod.handle, 0
                for p in range(row.ctypes.data, row.ctypes.data + 2 * op[1], 2):
                    status |= fn(h, p, 1, 1)
                assert status == 0
                out.append(row)
                after.append((mod.consumed(), mod.txoff_at(), mod.state()))
            else:
                _, a, _ = run_ops(mod, [op])
                accepted += list(a)
        samples = np.concatenate(out)[None, :]
        accepted = np.array(accepted, np.int32).reshape(-1, 1)
        after = tuple(np.array([a[k] for a in after]).reshape(-1, 1) for k in range(3))
    else:
        samples, accepted, after = run_ops(mod, g["ops"], chunk=chunk)
    check_samples(g, samples[0])
    check_outputs(g, accepted, after)
    mod.close()


def test_channels_are_independent():
    """fixtures of one parameter set side by side in one handle, and beside channels without text"""
    for names in (("rtty_s170_45_15", "rtty_altfigs", "rtty_lower_nocode", "rtty_idle", "rtty_eot"),
                  ("psk_125_high", "psk_125_eot", "psk_125_idle")):
        gs = [load_case(n) for n in names]
        first_gen = [next(op[1] for op in g["ops"] if op[0] == "gen") for g in gs]      # what follows a later op is not compared
        mod = make(gs[0], channels=len(gs) + 1)
        texts = [g["ops"][0][1] if g["ops"][0][0] == "put" else b"" for g in gs] + [b""]
        assert mod.put_text(texts).tolist() == [len(t) for t in texts]
        audio = mod.generate(max(first_gen))
        for c, g in enumerate(gs):
            check_samples(g, audio[c], upto=first_gen[c])
        idle = next(c for c, t in enumerate(texts) if not t)
        assert np.array_equal(audio[-1], audio[idle])
        mod.close()


def test_put_text_overflow_and_order():
    """a queue of `capacity` holds capacity - 1 characters; what is accepted comes out in order"""
    mod = digimod.PskModulator(3, psk.SPEED_125, capacity=8, host=True)
    assert mod.put_text([b"abcdefghij", b"", b"xyz"]).tolist() == [7, 0, 3]
    assert mod.put_text([b"k", b"0123456", b"uvwxyz"]).tolist() == [0, 7, 4]
    mod.generate(48000 + 384 * 25)              # the preamble of 125 bits and 25 bits more
    took = mod.consumed()
    assert (took > 0).all() and (took < 7).all()
    assert mod.put_text([b"ABCDEFGHIJ"] * 3).tolist() == took.tolist()      # exactly the room the modulator made
    mod.reset()
    mod.put_text([b"abcdefg", b"", b""])
    a = mod.generate(48000 + 3 * 384 * 12)
    accepted = int(mod.put_text([b"ABCDEFGHIJ", b"", b""])[0])
    assert 0 < accepted < 7
    b = mod.generate(150000)
    ref = digimod.PskModulator(1, psk.SPEED_125, capacity=64, host=True)
    ref.put_text(b"abcdefg" + b"ABCDEFGHIJ"[:accepted])
    want = ref.generate(a.shape[1] + b.shape[1])
    assert np.array_equal(np.concatenate([a[0], b[0]]), want[0])
    assert mod.consumed()[0] == ref.consumed()[0] == 7 + accepted
    mod.close()
    ref.close()


@pytest.mark.parametrize("name", LOOP_CASES)
def test_loopback(name):
    """own modulator, every fourth sample, own decoder: the bytes the reference decoder printed for
    the reference modulator's output at the recorded lead"""
    g = load_loop_case(name)
    mod = make(g)
    samples, _, _ = run_ops(mod, g["ops"])
    assert zlib.crc32(samples[0].tobytes()) == int(g["crc32"])
    audio = np.concatenate([np.zeros(g["lead"], np.float32), samples[0, ::4].astype(np.float32)])[None, :]
    if g["kind"] == "rtty":
        dec = rtty.RttyDecoder(1, g["shift_idx"], g["speed_idx"], g["stopbits_idx"], capacity=4096, host=True)
    else:
        dec = psk.PskDecoder(1, g["speed_idx"], capacity=4096, host=True)
    dec.process(np.ascontiguousarray(audio))
    assert dec.new_text()[0] == bytes(g["chars"])
    dec.close()
    mod.close()


def test_loopback_fixtures():
    assert LOOP_CASES == ["loop_psk_125", "loop_psk_31", "loop_rtty_s170_45"]
    for name in LOOP_CASES:
        g = load_loop_case(name)            # (the loader checks `verbatim` against the bytes; it does not ask for it)
        assert len(g["chars"]) > 0 and g["ops"][0][1] == bytes(g["message"])


def test_argument_errors():
    lib = U.load()
    h = C.c_void_p()
    for args in ((0, 1, 0, 1, 64), (4, -1, 0, 1, 64), (4, 6, 0, 1, 64), (4, 1, 2, 1, 64), (4, 1, 0, 3, 64), (4, 1, 0, 1, 7)):
        assert lib.uhsdr_rttymod_create_host(*args, C.byref(h)) == -1, args
        assert lib.uhsdr_rttymod_create(*args, None, C.byref(h)) == -1, args      # refused before any device call
    assert b"text_capacity" in lib.uhsdr_last_error()
    for args in ((0, 0, 64), (4, -1, 64), (4, 3, 64), (4, 0, 7)):
        assert lib.uhsdr_pskmod_create_host(*args, C.byref(h)) == -1, args
        assert lib.uhsdr_pskmod_create(*args, None, C.byref(h)) == -1, args
    assert lib.uhsdr_pskmod_create_host(4, 3, 64, C.byref(h)) == -1 and b"speed_idx" in lib.uhsdr_last_error()
    assert lib.uhsdr_pskmod_create_host(4, 0, 64, None) == -1
    x = np.zeros((4, 16), np.int16)
    text = np.zeros((4, 8), np.uint8)
    length = np.array([8, 0, 3, 1], np.int32)
    px, pt, pl = (C.c_void_p(a.ctypes.data) for a in (x, text, length))
    for kind, create in (("rttymod", lambda: lib.uhsdr_rttymod_create_host(4, 1, 0, 1, 8, C.byref(h))),
                         ("pskmod", lambda: lib.uhsdr_pskmod_create_host(4, 2, 8, C.byref(h)))):
        f = lambda name: getattr(lib, f"uhsdr_{kind}_{name}")     # noqa: E731
        assert create() == 0
        assert f("process_host")(h, None, 4, 16) == -1
        assert f("process_host")(h, px, 17, 16) == -2
        assert f("process_host")(h, px, -1, 16) == -2
        assert f("process")(h, px, 4, 16) == -1             # a host handle
        assert f("set_stream")(h, None) == -1
        assert f("put_text")(h, None, pl, 8, None) == -1
        assert f("put_text")(h, pt, None, 8, None) == -1
        assert f("put_text")(h, pt, pl, 7, None) == -2         # len[0] = 8 does not fit a row of 7
        assert f("put_text")(h, pt, pl, -1, None) == -2
        assert f("put_text")(h, pt, pl, 8, None) == 0          # accepted may be null
        assert f("process_host")(h, px, 16, 16) == 0
        assert f("process_host")(h, px, 0, 16) == 0
        assert f("destroy")(h) == 0
        assert f("process_host")(None, px, 4, 16) == -1
        assert f("put_text")(None, pt, pl, 8, None) == -1
        assert f("outputs")(None, None, None, None) == -1
        assert f("reset")(None) == -1
        assert f("destroy")(None) == -1
    assert lib.uhsdr_rttymod_start_tx(None) == -1 and lib.uhsdr_pskmod_prepare_tx(None) == -1
    assert lib.uhsdr_abi_version() == 9
