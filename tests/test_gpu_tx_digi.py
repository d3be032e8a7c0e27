"""DIGI transmit on the device (uhsdr_tx_* with the RTTY or BPSK modulator inside the chain: the
modulator kernel, tx_voice_digi, tx_iq) against the reference firmware's TxProcessor_Run in DIGI mode
(tests/golden/digimod_chain_*.npz, recorded by tools/digimod/make_digimod_golden.py at 32-frame
calls): the I/Q DAC frames and a_buffer[0] bit for bit."""
import ctypes as C

import numpy as np
import pytest

import uhsdr_amd as U
from uhsdr_amd import digimod

from digimod_cases import CHAIN_CASES, check_chain, load_chain_case
from test_gpu_tx import run_tx
from test_gpu_tx_precision import TOL, normwise
from test_tx_oracle import load_tx, tx_files

pytestmark = pytest.mark.gpu


def make_chain(g, channels, frames):
    chain = U.TxChain(U.tx_config_from_ref_args(g["args"]), channels=channels, frames=frames)
    if g["kind"] == "rtty":
        chain.set_rtty_mod(True, g["shift_idx"], g["speed_idx"], g["stopbits_idx"], g["capacity"])
    else:
        chain.set_psk_mod(True, g["speed_idx"], g["capacity"])
    return chain


def run_chain(g, frames, pipelined=False, precision=U.PRECISION_EXACT, texts=None, total=None):
    """the fixture's configuration at `frames` per call: iq int32 [C][n][2], a0 float32 [C][n], and
    the modulator's outputs at the end"""
    import torch
    texts = [g["text"], g["text"]] if texts is None else texts
    n = g["frames"] if total is None else total
    chain = make_chain(g, len(texts), frames)
    chain.set_pipelined(pipelined)
    chain.set_precision(precision)
    assert chain.mod_put_text(texts).tolist() == [len(t) for t in texts]
    iq = torch.zeros((n // frames, len(texts), frames, 2), dtype=torch.int32, device="cuda")
    a0 = torch.zeros((n // frames, len(texts), frames), dtype=torch.float32, device="cuda")
    for k in range(n // frames):
        chain.process_digi(iq[k], a0[k])
    chain.join()
    torch.cuda.synchronize()
    outs = chain.mod_outputs()
    chain.close()
    return (iq.permute(1, 0, 2, 3).reshape(len(texts), n, 2).cpu().numpy(), a0.permute(1, 0, 2).reshape(len(texts), n).cpu().numpy(), outs)


@pytest.mark.parametrize("frames,pipelined", [(32, False), (256, True), (2048, False)])
@pytest.mark.parametrize("name", CHAIN_CASES)
def test_chain_matches_reference_firmware(cuda, name, frames, pipelined):
    g = load_chain_case(name)
    iq, a0, (consumed, txoff_at, state) = run_chain(g, frames, pipelined)
    for c in range(2):
        check_chain(g, iq[c], a0[c])
    assert (consumed == g["consumed"]).all() and (state == g["state"]).all()
    assert ((txoff_at != digimod.NO_TXOFF) == bool(g["txoff"])).all()


@pytest.mark.parametrize("name", CHAIN_CASES)
def test_chain_fma_within_the_tx_tolerance(cuda, name):
    """the FMA precision of the Hilbert pair, pipelined, held to the tolerance the SSB modes are held
    to (test_gpu_tx_precision.py); a_buffer[0] is before the pair and stays exact"""
    g = load_chain_case(name)
    iq, a0, _ = run_chain(g, 2048, True, U.PRECISION_FMA)
    ref_iq, ref_a0, _ = run_chain(g, 2048, True, U.PRECISION_EXACT)
    check_chain(g, ref_iq[0], ref_a0[0])
    assert np.array_equal(a0.view(np.uint32), ref_a0.view(np.uint32))
    err = normwise(iq, ref_iq)
    print(f"tx digi fma {name}: max normwise {err:.3e}")
    assert err <= TOL
    assert not np.array_equal(iq, ref_iq), "FMA precision did not reach the kernel"


def test_chain_fixture_set():
    gs = [load_chain_case(n) for n in CHAIN_CASES]
    assert sorted((g["kind"], g["args"]["digilsb"]) for g in gs) == [("psk", 0), ("psk", 1), ("rtty", 0), ("rtty", 1)]
    assert sum(g["args"]["iqmode"] != 0 for g in gs) == 1          # pins "no translation"


@pytest.mark.parametrize("name", ["chain_rtty_usb", "chain_psk_usb"])
def test_130_channels_with_differing_texts(cuda, name):
    """every fifth channel carries the fixture's text and gives the fixture; the others carry other
    texts or none: equal texts give equal frames, different texts different ones, and every channel
    takes the characters a host modulator takes from the same text"""
    g = load_chain_case(name)
    other = [b"", b"the quick brown fox", b"73", g["text"][::-1]]
    texts = [g["text"] if c % 5 == 0 else other[c % 5 - 1] for c in range(130)]
    iq, a0, (consumed, _, state) = run_chain(g, 256, True, texts=texts)
    for c in (0, 65, 125):
        check_chain(g, iq[c], a0[c])
    for c in range(5, 130):
        assert np.array_equal(iq[c], iq[c % 5]) and np.array_equal(a0[c].view(np.uint32), a0[c % 5].view(np.uint32))
    assert len({iq[c].tobytes() for c in range(5)}) == 5
    if g["kind"] == "rtty":
        host = digimod.RttyModulator(130, g["shift_idx"], g["speed_idx"], g["stopbits_idx"], capacity=g["capacity"], host=True)
    else:
        host = digimod.PskModulator(130, g["speed_idx"], capacity=g["capacity"], host=True)
    host.put_text(texts)
    host.generate(g["frames"])
    assert np.array_equal(consumed, host.consumed()) and np.array_equal(state, host.state())
    host.close()


def test_reset_resets_the_modulator(cuda):
    g = load_chain_case("chain_psk_usb")
    import torch
    chain = make_chain(g, 3, 256)
    runs = []
    for _ in range(2):
        chain.mod_put_text(g["text"])
        iq = torch.zeros((8, 3, 256, 2), dtype=torch.int32, device="cuda")
        for k in range(8):
            chain.process_digi(iq[k])
        torch.cuda.synchronize()
        runs.append(iq.cpu().numpy())
        lib = U.load()
        assert lib.uhsdr_tx_prepare_run(chain.handle) == 0          # leaves the modulator alone
        chain.reset()
        assert (chain.mod_outputs()[0] == 0).all()
    assert np.array_equal(runs[0], runs[1]) and np.abs(runs[0]).max() > 0
    chain.close()


def test_refusals(cuda):
    import torch
    lib = U.load()
    g = load_chain_case("chain_rtty_usb")
    cfg = U.tx_config_from_ref_args(g["args"])
    chain = U.TxChain(cfg, channels=4, frames=64)
    iq = torch.zeros((4, 64, 2), dtype=torch.int32, device="cuda")
    # DIGI without a modulator
    with pytest.raises(U.UhsdrError) as e:
        chain.process_digi(iq)
    assert e.value.status == U.UHSDR_ARGUMENT_ERROR and "modulator" in str(e.value)
    for call in (chain.mod_start, chain.mod_outputs, lambda: chain.mod_put_text(b"x")):
        with pytest.raises(U.UhsdrError):
            call()
    # TUNE: the dvmode branch never looks at it
    with pytest.raises(U.UhsdrError) as e:
        chain.set_tune(U.TUNE_SINGLE)
    assert e.value.status == U.UHSDR_ARGUMENT_ERROR
    # one modulator at a time, in either order; bad arguments as the stand-alone create
    chain.set_rtty_mod(True)
    with pytest.raises(U.UhsdrError) as e:
        chain.set_psk_mod(True)
    assert e.value.status == U.UHSDR_ARGUMENT_ERROR and "one modulator" in str(e.value)
    chain.process_digi(iq)
    chain.set_rtty_mod(False)
    chain.set_psk_mod(True, 2, 8)
    with pytest.raises(U.UhsdrError):
        chain.set_rtty_mod(True)
    with pytest.raises(U.UhsdrError):
        chain.set_psk_mod(True, 3, 64)
    with pytest.raises(U.UhsdrError):
        chain.set_psk_mod(True, 0, 7)
    assert chain.mod_put_text(b"0123456789").tolist() == [7] * 4
    chain.process_digi(iq)
    torch.cuda.synchronize()
    assert int(iq.abs().max()) > 0
    chain.close()
    # the five calls on a handle of another mode, and on none
    ssb = U.TxChain(U.default_tx_config(), channels=2, frames=64)
    for call in (lambda: ssb.set_rtty_mod(True), lambda: ssb.set_psk_mod(True), ssb.mod_start, ssb.mod_outputs):
        with pytest.raises(U.UhsdrError):
            call()
    ssb.close()
    assert lib.uhsdr_tx_set_rtty_mod(None, 1, 1, 0, 1, 64) == -1 and lib.uhsdr_tx_mod_start(None) == -1
    # the USB I/Q source with DIGI
    h = C.c_void_p()
    bad = U.tx_config_from_ref_args(dict(g["args"], txsrc=4))
    assert lib.uhsdr_tx_create(C.byref(bad), 2, 64, None, C.byref(h)) != 0


def test_ssb_handle_beside_a_digi_handle(cuda):
    """the voice kernels are untouched: with a DIGI handle alive in the process, an SSB handle still
    gives the reference firmware's frames"""
    import torch
    g = load_chain_case("chain_psk_lsb")
    digi = make_chain(g, 2, 256)
    iq = torch.zeros((2, 256, 2), dtype=torch.int32, device="cuda")
    digi.process_digi(iq)
    t = load_tx([p for p in tx_files() if p.endswith("tx_usb.npz")][0])
    got_iq, got_a0 = run_tx(U.tx_config_from_ref_args(t["args"]), t["audio"], 256, t["args"])
    np.testing.assert_array_equal(got_a0.view(np.uint32), t["a0"].view(np.uint32))
    np.testing.assert_array_equal(got_iq, t["iq"])
    digi.process_digi(iq)
    torch.cuda.synchronize()
    digi.close()
