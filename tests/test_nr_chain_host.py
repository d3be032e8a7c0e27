"""The noise reduction stage of the receive chain, without a device.

The recordings of tests/golden/nrchain_*.npz hold each 8-sample block that entered and left the
firmware's AudioDriver_RxProcessorNoiseReduction inside its whole receive chain.  The stand-alone
12 ksps stream (uhsdr_nr_process_host) on what entered gives what left, bit for bit, at every call
size: the module uhsdr_rx_set_nr runs between its two kernels is the chain's stage, and the
recordings are pinned.  Then the refusals of the two entry points that need no device."""
import ctypes as C

import numpy as np
import pytest

import uhsdr_amd as U
from nr_chain_cases import CASES, load_case, nr_cfg, same_bits
from uhsdr_amd import nr


def stream(g, step):
    x = np.ascontiguousarray(g["nr_in"])
    p = nr.NrProcessor(x.shape[0], nr_cfg(g), host=True)
    out = np.empty_like(x)
    for o in range(0, x.shape[1], step):
        xi = np.ascontiguousarray(x[:, o:o + step])
        yo = np.full_like(xi, np.nan)
        p.process(xi, yo)
        out[:, o:o + step] = yo
    state = p.state()
    p.close()
    return out, state


@pytest.mark.parametrize("name", CASES)
def test_stream_module_is_the_chains_stage(name):
    g = load_case(name)
    nd = g["nr_in"].shape[1]
    assert g["nr_in"].shape == g["nr_out"].shape == (2, nd) and g["audio"].shape == (2, 4 * nd) and g["iq"].shape == (2, 4 * nd, 2)
    decimated = g["nr"]["width_hz"] < 2701
    assert nd >= 30 * 128 * (2 if decimated else 1)          # past the 20-frame start-up and the FIFO's two frames
    states = []
    for step in (8, 128, nd):                                # the firmware's block, 512-frame calls, one call
        out, state = stream(g, step)
        assert same_bits(out, g["nr_out"]), (name, step, int(np.argmax(out.view(np.uint32) != g["nr_out"].view(np.uint32))))
        states.append(state)
    for s in states[1:]:
        assert all(same_bits(a, b) for a, b in zip(s, states[0]))
    if not g["nr"]["nr_bypass"]:
        assert (states[0][0] == 3).all()                     # the noise reduction runs: first_time 3


def test_the_two_recordings_of_a_case_differ():
    for name in CASES:
        g = load_case(name)
        assert not np.array_equal(g["iq"][0], g["iq"][1]) and not same_bits(g["audio"][0], g["audio"][1]), name


def test_null_handle():
    lib = U.load()
    cfg = nr.nr_config()
    assert lib.uhsdr_rx_set_nr(None, C.byref(cfg)) == U.UHSDR_ARGUMENT_ERROR == -1
    assert lib.uhsdr_rx_set_nr(None, None) == -1
    five = [np.zeros(1, np.int32).ctypes.data_as(C.c_void_p)] * 5
    assert lib.uhsdr_rx_nr_state(None, *five) == -1
    assert b"noise reduction" in lib.uhsdr_last_error()
