"""The CPU oracle on the edge inputs (synth.edge_iq / edge_audio: silence, signal / silence /
signal, full-scale impulses and square waves, +-3 LSB noise, all 32 input bits in use) against the
reference firmware's recorded output (tests/golden/rxedge_*.npz, txedge_*.npz), bit for bit: every
32-frame call's crc32 of a_buffer[1], a_buffer[0] and the codec frames, and the stored windows.

In the silence the recursive stages (IIR lattices, biquads, AGC, LMS notch, interpolator, FM
filters, TX ALC and band-pass) decay into the denormals and stay in small limit cycles until the
signal returns: tens of thousands of denormal samples per row, counted here from the oracle's own
output and held to the count recorded from the reference.  This is what lets the device tests
(test_gpu_edge.py) use the oracle as the reference's stand-in on inputs derived from these rows."""
import numpy as np
import pytest

import edge_util as E
import oracle
import uhsdr_amd as U
from golden_util import assert_bitexact
from test_cw_oracle import cw_blocks


def test_edge_fixtures_present_and_to_the_point():
    assert len(E.RX_NAMES) == 14 and len(E.TX_NAMES) == 4
    for name in E.RX_NAMES:
        E.load_rx(name)
    for name in E.TX_NAMES:
        E.load_tx(name)


@pytest.mark.parametrize("name", E.RX_NAMES)
def test_oracle_rx_matches_reference(name):
    g = E.load_rx(name)
    plan = U.build_plan(E.rx_config(g))
    R = len(g["kinds"])
    o = oracle.OracleRx(plan, R)
    if "cw_energy" in g:
        assert plan.cw_enabled
        a1, dst, sig, en = oracle.rx_process_cw(o, g["rows"], cw_blocks(plan, g["frames"]), threads=R)
        a0 = None
        assert en.shape == g["cw_energy"].shape
        assert_bitexact(en, g["cw_energy"], "Goertzel energy")
        np.testing.assert_array_equal(sig, g["cw_signal"])
    else:
        a1, a0, dst = o.process2(g["rows"], threads=R)
    for r, kind in enumerate(g["kinds"]):
        bad = E.mismatch(g, r, {"a1": a1[r], "a0": None if a0 is None else a0[r], "dst": dst[r]})
        assert bad is None, f"{name} {kind}: {bad}"
        assert E.denormals(a1[r]) == int(g["denormal_a1"][r])
        assert np.abs(a1[r]).max() == g["peak_a1"][r]


@pytest.mark.parametrize("name", E.TX_NAMES)
def test_oracle_tx_matches_reference(name):
    g = E.load_tx(name)
    R = len(g["kinds"])
    iq, a0 = oracle.OracleTx(U.build_tx_plan(E.tx_config(g)), R).process(g["rows"], threads=R)
    for r, kind in enumerate(g["kinds"]):
        bad = E.mismatch(g, r, {"a0": a0[r], "iq": iq[r]})
        assert bad is None, f"{name} {kind}: {bad}"
        assert E.denormals(a0[r]) == int(g["denormal_a0"][r])


@pytest.mark.parametrize("name", ["p48_usb", "p1_fm"])
def test_oracle_call_size_does_not_matter_in_the_silence(name):
    """32-frame calls against 2048-frame calls on the burst row: the state the oracle carries from
    call to call holds the denormals as they are"""
    g = E.load_rx(name)
    r = g["kinds"].index("burst")
    iq = np.ascontiguousarray(g["rows"][r:r + 1])
    plan = U.build_plan(E.rx_config(g))
    outs = []
    for N in (32, 2048):
        o = oracle.OracleRx(plan, 1)
        parts = [o.process2(np.ascontiguousarray(iq[:, k:k + N])) for k in range(0, g["frames"], N)]
        outs.append([np.concatenate([p[i] for p in parts], axis=1) for i in range(3)])
    assert_bitexact(outs[0][0], outs[1][0], "a1, 32- against 2048-frame calls")
    assert_bitexact(outs[0][1], outs[1][1], "a0, 32- against 2048-frame calls")
    np.testing.assert_array_equal(outs[0][2], outs[1][2])
    assert E.mismatch(g, r, {"a1": outs[0][0][0], "dst": outs[0][2][0]}) is None


def test_checker_sees_one_flipped_bit():
    """the comparison the device tests rely on: one low bit of one denormal sample, inside a stored
    window or between them, in a full row or in a single call, is reported with its call"""
    g = E.load_rx("p48_usb")
    r = g["kinds"].index("burst")
    a1, _, dst = oracle.OracleRx(U.build_plan(E.rx_config(g)), 1).process2(np.ascontiguousarray(g["rows"][r:r + 1]))
    a1, dst = a1[0], dst[0]
    assert E.mismatch(g, r, {"a1": a1, "dst": dst}) is None
    start = int(g["win_start"][r][1])
    den = np.flatnonzero((np.abs(a1) > 0) & (np.abs(a1) < E.FLT_MIN))
    assert den[0] == start
    for frame in (int(den[0]), int(den[den > start + 40000][0])):
        bent = a1.copy()
        bent.view(np.uint32)[frame] ^= 1
        bad = E.mismatch(g, r, {"a1": bent, "dst": dst})
        assert bad is not None and bad[:2] == (frame // 32, "a1")
        lo = frame // 32 * 32
        assert E.mismatch(g, r, {"a1": bent[lo:lo + 32]}, frame0=lo)[0] == frame // 32
        assert E.mismatch(g, r, {"a1": a1[lo:lo + 32]}, frame0=lo) is None
        text = E.describe(g, r, 7, bad, {"a1": bent})
        assert f"call {frame // 32}" in text and "oracle a1" in text
    bent = dst.copy()
    bent[100, 1] ^= 1 << 16
    assert E.mismatch(g, r, {"a1": a1, "dst": bent})[:2] == (3, "dst")
