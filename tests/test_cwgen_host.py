"""The CW generator's block and sample functions on the CPU (uhsdr_cwgen_process_host) against the
recordings of the reference firmware's CwGen_Process (tests/golden/cwgen_*.npz): every block's flags,
cw_state, key_timer, sm_tbl_ptr, port_state and DDS accumulator, the crc32 of every block of I and of
Q, three raw windows over edges, the characters taken and the bytes echoed.  Everything is
bit-equal."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from uhsdr_amd import _abi, cwgen

from cwgen_cases import CASES, GOLDEN, check_run, load_case, make, run_host

ROOT = GOLDEN.rsplit("/tests/", 1)[0]


def test_fixtures_present():
    kinds = ("straight_", "iam_a", "iam_b", "ultimate", "timing_", "tone_", "text_", "echo", "set_speed")
    assert all(any(n.startswith(k) for n in CASES) for k in kinds), CASES
    assert len([n for n in CASES if n.startswith("timing_")]) == 9 and len([n for n in CASES if n.startswith("tone_")]) == 4


def test_table_file_is_what_the_fixture_gives():
    subprocess.run([sys.executable, f"{ROOT}/tools/cwgen/gen_cwgen_tables.py", "--check"], check=True)


@pytest.mark.parametrize("name", CASES)
def test_single_call(name):
    """one call between two events"""
    g = load_case(name)
    check_run(g, run_host(g))


@pytest.mark.parametrize("name", CASES)
def test_block_calls(name):
    """32-sample calls, the keyer's words after every block"""
    g = load_case(name)
    check_run(g, run_host(g, each_block=True))


@pytest.mark.parametrize("name", ["iam_b", "text_sentence", "straight_repress", "echo"])
def test_odd_calls_among_idle_channels(name):
    """calls of 7 blocks, as the middle one of three channels"""
    g = load_case(name)
    check_run(g, run_host(g, chunk=7, channels=3, at=1))


def test_channels_are_independent():
    """every case of one setting at once, a channel each, against its own recording"""
    names = ["tone_750", "text_sentence", "text_mid_element", "text_paddle"]
    gs = [load_case(n) for n in names]
    assert len({tuple(g[k] for k in ("mode", "speed", "weight", "reverse", "rx_delay", "sidetone", "capacity")) for g in gs}) == 1
    B = max(g["blocks"] for g in gs)
    gen = make(gs[0], channels=len(gs))
    keys = np.zeros((len(gs), B), np.uint8)
    for c, g in enumerate(gs):
        keys[c, :g["blocks"]] = g["keys"]
    gen.put_text([g["events"][0][1][1] if g["events"] and g["events"][0][0] == 0 else b"" for g in gs])
    i, q = gen.generate(keys)
    from cwgen_cases import check_samples
    for c, g in enumerate(gs):
        later = [b for b, _ in g["events"] if b > 0]
        check_samples(g, i[c], q[c], blocks=min(later) if later else g["blocks"])
    gen.close()


def test_reset_reproduces_the_run():
    g = load_case("text_sentence")
    gen = make(g)
    runs = []
    for _ in range(2):
        assert gen.put_text(g["ops"][0][1]).tolist() == [len(g["ops"][0][1])]
        i, q = gen.generate(g["keys"][None, :])
        runs.append((i, q, gen.flags(), gen.consumed(), gen.echo()[0]))
        gen.reset()
        assert gen.consumed()[0] == 0 and gen.echo_total()[0] == 0 and all((v == 0).all() for v in gen.peek().values())
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert runs[0][4] == g["echo"]
    gen.close()


def test_queue_capacity_and_closure():
    gen = cwgen.CwGenerator(2, mode=cwgen.IAM_B, speed=48, capacity=8, echo_capacity=8, host=True)
    assert gen.put_text([b"0123456789", b"abc"]).tolist() == [7, 3]
    assert gen.put_text([b"x", b"defgh"]).tolist() == [0, 4]
    # a closing key line empties the queue of its channel only
    keys = np.zeros((2, 1), np.uint8)
    keys[0, 0] = cwgen.DIT
    gen.generate(keys)
    assert gen.consumed().tolist() == [7, 1]
    assert gen.put_text([b"0123456789", b""]).tolist() == [7, 0]
    gen.close()


def test_echo_ring_wraps():
    """nine E through a ring of 8 bytes: the last eight printed remain, oldest first"""
    gen = cwgen.CwGenerator(1, mode=cwgen.IAM_B, speed=48, capacity=16, echo_capacity=8, host=True)
    gen.put_text(b"EEEEEEEEE")
    gen.generate(np.zeros((1, 4000), np.uint8))
    assert gen.echo_total()[0] == 10 and gen.echo()[0] == b"EEEEEEE "
    gen.close()


def test_argument_errors():
    lib = _abi.load()
    h = C.c_void_p()

    def cfg(**kw):
        d = dict(keyer_mode=0, keyer_speed=20, keyer_weight=100, paddle_reverse=0, rx_delay=8, sidetone_freq=750)
        d.update(kw)
        return cwgen._Config(*[d[k] for k, _ in cwgen._Config._fields_])

    for bad in (dict(keyer_mode=4), dict(keyer_mode=-1), dict(keyer_speed=4), dict(keyer_speed=49), dict(keyer_weight=49), dict(keyer_weight=151),
                dict(rx_delay=51), dict(rx_delay=-1), dict(sidetone_freq=399), dict(sidetone_freq=1001)):
        assert lib.uhsdr_cwgen_create_host(1, C.byref(cfg(**bad)), 16, 16, C.byref(h)) == _abi.UHSDR_ARGUMENT_ERROR, bad
        assert lib.uhsdr_last_error()
    ok = cfg()
    assert lib.uhsdr_cwgen_create_host(0, C.byref(ok), 16, 16, C.byref(h)) == _abi.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_cwgen_create_host(1, C.byref(ok), 7, 16, C.byref(h)) == _abi.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_cwgen_create_host(1, C.byref(ok), 16, 7, C.byref(h)) == _abi.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_cwgen_create_host(1, None, 16, 16, C.byref(h)) == _abi.UHSDR_ARGUMENT_ERROR
    gen = cwgen.CwGenerator(2, host=True)
    keys, i, q = np.zeros((2, 2), np.uint8), np.zeros((2, 64), np.float32), np.zeros((2, 64), np.float32)
    p = [x.ctypes.data_as(C.c_void_p) for x in (keys, i, q)]
    assert lib.uhsdr_cwgen_process_host(gen.handle, *p, 33, 64) == _abi.UHSDR_LENGTH_ERROR        # not whole blocks
    assert lib.uhsdr_cwgen_process_host(gen.handle, *p, 96, 64) == _abi.UHSDR_LENGTH_ERROR        # past the row
    assert lib.uhsdr_cwgen_process_host(gen.handle, None, p[1], p[2], 64, 64) == _abi.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_cwgen_process(gen.handle, *p, 64, 64) == _abi.UHSDR_ARGUMENT_ERROR           # a host handle
    assert lib.uhsdr_cwgen_set_speed(gen.handle, 60, 100) == _abi.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_cwgen_set_stream(gen.handle, None) == _abi.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_cwgen_process_host(gen.handle, *p, 0, 64) == _abi.UHSDR_OK
    gen.close()
