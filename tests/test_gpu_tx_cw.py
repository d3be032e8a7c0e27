"""CW inside the transmit chain (uhsdr_tx_* with dmod_mode DEMOD_CW, kernel tx_cw) against the
recordings of the reference's TxProcessor_Run (tests/golden/cwgen_chain_*.npz): the int32 I/Q frames
and a_buffer[0] of every 32-frame call, the flags, the characters taken and the echo, bit for bit.
Even channels run the recording, odd channels have open key lines and no text."""
import ctypes as C
import functools

import numpy as np
import pytest

import uhsdr_amd as U
from uhsdr_amd import _abi

from cwgen_cases import CHAIN_CASES, ECHO_CAPACITY, check_chain, load_chain_case

pytestmark = pytest.mark.gpu

CHANNELS = 5


def config(g, **more):
    kw = {_abi.TX_ARG_MAP[k]: v for k, v in g["args"].items()}
    kw.update(cw_lsb=g["cw_lsb"], cw_keyer_mode=g["mode"], cw_keyer_speed=g["speed"], cw_keyer_weight=g["weight"],
              cw_paddle_reverse=g["reverse"], cw_rx_delay=g["rx_delay"], cw_sidetone_freq=g["sidetone"])
    kw.update(more)
    return _abi.default_tx_config(**kw)


def run_chain(g, frames, torch, channels=CHANNELS, setup=None, upto=None):
    """the recording in calls of `frames` frames; returns iq [C][n][2], a0 [C][n], flags [C][n/32], the outputs"""
    chain = U.TxChain(config(g), channels=channels, frames=frames)
    chain.set_cw_keyer(capacity=g["capacity"], echo_capacity=ECHO_CAPACITY)
    if setup:
        setup(chain)
    n = g["frames"] if upto is None else upto
    per = frames // 32
    keys = np.zeros((n // frames, channels, per), np.uint8)
    keys[:, 0::2, :] = g["keys"][:n // 32].reshape(n // frames, 1, per)
    dkeys = torch.from_numpy(keys).cuda()
    assert chain.cw_put_text([g["text"] if c % 2 == 0 else b"" for c in range(channels)]).tolist() == [len(g["text"]) * (c % 2 == 0) for c in range(channels)]
    iq = torch.full((n // frames, channels, frames, 2), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    a0 = torch.full((n // frames, channels, frames), 7.0, dtype=torch.float32, device="cuda")
    flags = []
    t0, tn = g["tune"] if g["tune"] else (-1, 0)
    for k in range(n // frames):
        call = k * per                      # the recording's 32-frame call this one starts at
        if call == t0:
            chain.set_tune(_abi.TUNE_SINGLE)
        if t0 >= 0 and call == t0 + tn:
            chain.set_tune(_abi.TUNE_OFF)
        chain.cw_keys(dkeys[k])
        chain.process_cw(iq[k], a0[k])
        if per == 1 and k % 64:
            continue                        # the flags of every 64th 32-frame call only: each look waits for the device
        torch.cuda.synchronize()
        flags.append((k, chain.cw_outputs()[0]))
    torch.cuda.synchronize()
    out = chain.cw_outputs()
    chain.close()
    iq = iq.cpu().numpy().transpose(1, 0, 2, 3).reshape(channels, n, 2)
    a0 = a0.cpu().numpy().transpose(1, 0, 2).reshape(channels, n)
    return iq, a0, flags, out


def check_all(g, frames, iq, a0, flags, out):
    per = frames // 32
    for c in range(iq.shape[0]):
        if c % 2 == 0:
            check_chain(g, iq[c], a0[c])
            for k, f in flags:
                assert np.array_equal(f[c], g["flags"][k * per:(k + 1) * per]), (g["name"], c, k)
            assert out[1][c] == g["consumed"] and bytes(out[2][c, :out[3][c]]) == g["echo"]
        else:
            # nothing keyed: silence, except in TUNE, where every channel sends the tone
            quiet = np.ones(g["frames"], bool)
            if g["tune"]:
                quiet[32 * g["tune"][0]:32 * (g["tune"][0] + g["tune"][1])] = False
                assert np.array_equal(iq[c][~quiet], iq[0][~quiet]) and np.array_equal(a0[c][~quiet], a0[0][~quiet])
            assert not iq[c][quiet].any() and not a0[c][quiet].any() and out[1][c] == 0 and out[3][c] == 0


@pytest.mark.parametrize("frames", [32, 256, 2048])
@pytest.mark.parametrize("name", CHAIN_CASES)
def test_chain_fixtures(cuda, name, frames):
    import torch
    g = load_chain_case(name)
    check_all(g, frames, *run_chain(g, frames, torch))


def test_two_waves_and_a_partial_one(cuda):
    """130 channels: two full waves and two lanes of a third"""
    import torch
    g = load_chain_case("chain_gains")
    check_all(g, 2048, *run_chain(g, 2048, torch, channels=130))


def test_cases_present():
    assert len(CHAIN_CASES) == 4
    gs = [load_chain_case(n) for n in CHAIN_CASES]
    assert any(g["cw_lsb"] and g["mode"] == 2 for g in gs) and any(g["tune"] for g in gs) and any(g["text"] and g["mode"] != 2 for g in gs)
    assert any(g["args"].get("txgi", 1.0) != 1.0 and g["args"].get("txpwr", 0.5) != 0.5 for g in gs)


@functools.lru_cache(maxsize=None)
def plain(name):
    import torch
    g = load_chain_case(name)
    return run_chain(g, 256, torch, upto=16384)


@pytest.mark.parametrize("what", ["pipelined", "fma"])
def test_pipelined_and_precision_change_nothing(cuda, what):
    import torch
    g = load_chain_case("chain_gains")
    setup = (lambda ch: ch.set_pipelined(True)) if what == "pipelined" else (lambda ch: ch.set_precision(_abi.PRECISION_FMA))
    iq, a0, _, out = run_chain(g, 256, torch, upto=16384, setup=setup)
    ref = plain("chain_gains")
    assert np.array_equal(iq, ref[0]) and np.array_equal(a0.view(np.uint32), ref[1].view(np.uint32)) and np.array_equal(out[2], ref[3][2])
    assert np.abs(iq).max() > 0


def test_reset_and_prepare_run(cuda):
    """uhsdr_tx_reset resets the keyer (the run repeats); uhsdr_tx_prepare_run leaves it alone (the run goes on)"""
    import torch
    g = load_chain_case("chain_usb_text")
    chain = U.TxChain(config(g), channels=2, frames=256)
    chain.set_cw_keyer(capacity=g["capacity"], echo_capacity=ECHO_CAPACITY)
    keys = torch.zeros((2, 8), dtype=torch.uint8, device="cuda")
    chain.cw_keys(keys)

    def calls(k):
        iq = torch.zeros((k, 2, 256, 2), dtype=torch.int32, device="cuda")
        for j in range(k):
            chain.process_cw(iq[j])
        torch.cuda.synchronize()
        return iq.cpu().numpy().transpose(1, 0, 2, 3).reshape(2, k * 256, 2)

    chain.cw_put_text([g["text"], b""])
    first = calls(16)
    _abi.check(chain.lib.uhsdr_tx_prepare_run(chain.handle), "uhsdr_tx_prepare_run")
    second = calls(16)
    whole = np.concatenate([first, second], axis=1)[0]
    crc = np.array([__import__("zlib").crc32(np.ascontiguousarray(whole[k:k + 32]).tobytes()) for k in range(0, len(whole), 32)], np.uint32)
    assert np.array_equal(crc, g["iq_crc"][:len(crc)])
    chain.reset()
    assert chain.cw_outputs()[1].tolist() == [0, 0] and chain.cw_outputs()[3].tolist() == [0, 0]
    chain.cw_put_text([g["text"], b""])
    assert np.array_equal(calls(16), first)
    chain.close()


def test_refused_combinations(cuda):
    import torch
    lib = _abi.load()
    E = _abi.UHSDR_ARGUMENT_ERROR
    h = C.c_void_p()
    # the USB I/Q source with CW, and keyer settings out of range
    for bad in (dict(audio_source=_abi.TX_AUDIO_DIGIQ), dict(cw_keyer_speed=4), dict(cw_keyer_mode=4), dict(cw_sidetone_freq=1200), dict(cw_rx_delay=51)):
        cfg = _abi.default_tx_config(dmod_mode=_abi.DEMOD_CW, **bad)
        assert lib.uhsdr_tx_create(C.byref(cfg), 2, 32, None, C.byref(h)) == E, bad
        assert lib.uhsdr_last_error()
    cw = U.TxChain(channels=2, frames=32, dmod_mode=_abi.DEMOD_CW)
    ssb = U.TxChain(channels=2, frames=32)
    iq = torch.zeros((2, 32, 2), dtype=torch.int32, device="cuda")
    keys = torch.zeros((2, 1), dtype=torch.uint8, device="cuda")
    null = C.c_void_p(0)
    # the CW calls on a handle of another mode
    assert lib.uhsdr_tx_set_cw_keyer(ssb.handle, 16, 16) == E
    assert lib.uhsdr_tx_cw_keys(ssb.handle, C.c_void_p(keys.data_ptr())) == E
    assert lib.uhsdr_tx_cw_set_speed(ssb.handle, 20, 100) == E
    assert lib.uhsdr_tx_cw_put_text(ssb.handle, null, null, 0, null) == E
    assert lib.uhsdr_tx_cw_outputs(ssb.handle, None, None, None, None, None) == E
    # the modulator calls on a CW handle
    assert lib.uhsdr_tx_set_rtty_mod(cw.handle, 1, 1, 0, 1, 64) == E
    assert lib.uhsdr_tx_set_psk_mod(cw.handle, 1, 0, 64) == E
    assert lib.uhsdr_tx_mod_start(cw.handle) == E
    # processing before the keyer exists, and before the key lines are set
    assert lib.uhsdr_tx_process(cw.handle, None, C.c_void_p(iq.data_ptr()), None) == E
    assert lib.uhsdr_tx_cw_set_speed(cw.handle, 20, 100) == E
    cw.set_cw_keyer(16, 16)
    assert lib.uhsdr_tx_process(cw.handle, None, C.c_void_p(iq.data_ptr()), None) == E
    assert b"key lines" in lib.uhsdr_last_error()
    assert lib.uhsdr_tx_cw_set_speed(cw.handle, 60, 100) == E
    # TUNE needs no key lines; with them set, a call runs
    cw.set_tune(_abi.TUNE_SINGLE)
    cw.process_cw(iq)
    torch.cuda.synchronize()
    assert iq.cpu().numpy().any()
    cw.set_tune(_abi.TUNE_OFF)
    cw.cw_keys(keys)
    cw.process_cw(iq)
    torch.cuda.synchronize()
    assert not iq.cpu().numpy().any()
    cw.close()
    ssb.close()
