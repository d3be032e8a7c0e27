"""The signal meter on the device against the reference firmware's recordings (tests/meter_cases.py):
the stand-alone kernel meter_frames on every case, the meter as the spectrum kernel's epilogue on the
cases whose frames are a spectrum recording (driven from that recording's I/Q, at call sizes that
complete none, one, four and eight frames), ragged batches against the host twin fed the CPU
oracle's magnitudes, reset, and attach / detach.  Bit for bit on all six outputs."""
import os

import numpy as np
import pytest

import meter_cases as mc
import oracle
import uhsdr_amd as U
from golden_util import assert_bitexact
from uhsdr_amd import meter, synth

pytestmark = pytest.mark.gpu

SENTINEL = -7           # what a row holds before a call: no output of any case


def device_rows(C, F):
    """the six rows as tensors (the uint32 row as int32: the same four bytes), filled with SENTINEL"""
    import torch
    return {name: torch.full((C, F), SENTINEL, dtype=torch.float32 if dt is np.float32 else torch.int32, device="cuda")
            for name, dt in meter.OUTPUTS}


def to_host(rows, n=None):
    types = dict(meter.OUTPUTS)
    return {k: np.ascontiguousarray(v.cpu().numpy()[:, :n]).view(types[k]) for k, v in rows.items()}


def untouched(rows):
    return all(bool((v == SENTINEL).all()) for v in rows.values())


def run_frames(g, m=None, first=0, frames=None):
    import torch
    m = m or U.Meter(g["channels"], mc.config_of(g))
    last = g["frames"] if frames is None else first + frames
    rows = device_rows(g["channels"], last - first)
    m.process_mag(torch.from_numpy(np.ascontiguousarray(g["mag"][:, first:last])).cuda(),
                  torch.from_numpy(np.ascontiguousarray(g["cw_signal"][:, first:last])).cuda(), **rows)
    m.synchronize()
    return to_host(rows)


@pytest.mark.parametrize("name", mc.CASES)
def test_meter_frames_matches_reference_firmware(cuda, name):
    g = mc.load_case(name)
    mc.check_rows(g, run_frames(g), what="meter_frames")


def test_meter_frames_call_granularity_and_state(cuda):
    g = mc.load_case("cw300_p9_lsb")
    m = U.Meter(g["channels"], mc.config_of(g))
    for first in range(0, g["frames"], 3):
        n = min(3, g["frames"] - first)
        mc.check_rows(g, run_frames(g, m, first, n), first=first, what="calls of 3")
    st = m.state()
    for k in mc.OUTPUTS:
        assert mc.same(st[k], g[k][:, -1]).all(), k


def run_fused(cfg, mcfg, iq, per_call, want_spec, cw=None):
    """the spectrum with a meter attached over iq [C][n][2] in calls of per_call input frames: the
    meter's rows, mag and avg of every completed frame; a call that completes nothing must write nothing"""
    import torch
    C, n, _ = iq.shape
    spec = U.Spectrum(cfg, channels=C, frames=per_call)
    m = U.Meter(C, mcfg)
    F = spec.frames_out
    rows = device_rows(C, F)
    d_cw = torch.from_numpy(np.ascontiguousarray(cw)).cuda() if cw is not None else None
    spec.set_meter(m, d_cw, **rows)
    d_mag = torch.full(spec.out_shape, -1.0, dtype=torch.float32, device="cuda") if want_spec else None
    d_avg = torch.full(spec.out_shape, -1.0, dtype=torch.float32, device="cuda") if want_spec else None
    d_iq = torch.empty((C, per_call, 2), dtype=torch.int32, device="cuda")
    out = {k: [] for k in mc.OUTPUTS}
    mags, avgs, idle = [], [], 0
    for off in range(0, n, per_call):
        d_iq.copy_(torch.from_numpy(np.ascontiguousarray(iq[:, off:off + per_call])))
        nf = spec.process(d_iq, d_mag, d_avg)
        torch.cuda.synchronize()
        if nf == 0:
            idle += 1
            if idle <= 3:           # reading all rows back after each of hundreds of calls would only slow the test
                assert untouched(rows), f"a call that completed no frame wrote (input frame {off})"
            continue
        for k, v in to_host(rows, nf).items():
            out[k].append(v)
        if want_spec:
            mags.append(d_mag[:, :nf].cpu().numpy())
            avgs.append(d_avg[:, :nf].cpu().numpy())
        for v in rows.values():
            v.fill_(SENTINEL)
    state = m.state()
    spec.close()
    m.close()
    cat = lambda xs: np.concatenate(xs, axis=1) if xs else None  # noqa: E731
    return {k: cat(v) for k, v in out.items()}, cat(mags), cat(avgs), state, idle


@pytest.mark.parametrize("per_call,want_spec", [(32, False), (256, True), (1024, False), (1024, True), (2048, True)])
@pytest.mark.parametrize("name", mc.SPEC_CASES)
def test_fused_meter_matches_reference_firmware(cuda, name, per_call, want_spec):
    g = mc.load_case(name)
    cfg = U.spectrum_config_from_ref_args(g["spec_args"])
    rows, mag, avg, state, idle = run_fused(cfg, mc.config_of(g), g["iq"], per_call, want_spec)
    n = g["spec_frames"]
    assert rows["dbm"].shape == (g["channels"], n)
    mc.check_rows(g, rows, frames=n, what=f"fused, calls of {per_call}")
    for k in mc.OUTPUTS:
        assert mc.same(state[k], g[k][:, n - 1]).all(), k
    if per_call == 32:
        assert idle > 0             # the accumulate path ran
    if want_spec:
        with np.load(os.path.join(mc.GOLDEN, f"spec_{g['spec']}.npz")) as z:
            assert_bitexact(mag, z["mag"], "FFT_MagData beside the meter")
            assert_bitexact(avg, z["avg"], "FFT_AVGData beside the meter")


@pytest.mark.parametrize("L,channels,mode", [(256, 65, "am"), (512, 130, "cw"), (256, 130, "usb"), (512, 65, "am")])
def test_ragged_batches_match_host_twin_on_oracle_magnitudes(cuda, L, channels, mode):
    import torch
    cfg = U.default_spectrum_config(fft_len=L, spectrum_filter=3, iq_gain_i=1.01, iq_gain_q=0.99, iq_phase_balance=-0.003)
    mcfg = U.meter_config(fft_len=L, tune_old=14070000, **{
        "am": dict(dmod_mode=U.DEMOD_AM, filter_path=2), "cw": dict(dmod_mode=U.DEMOD_CW, filter_path=9), "usb": {}}[mode])
    iq = synth.ssb_iq(np.arange(channels), 7, 4096)
    om, _ = oracle.OracleSpectrum(U.build_spectrum_plan(cfg), channels).process(iq, threads=8)
    F = om.shape[1]
    cw = (np.arange(channels * F).reshape(channels, F) % 3 != 0).astype(np.uint8)
    want = U.Meter(channels, mcfg, host=True).process_mag_host(np.ascontiguousarray(om), cw)
    # the epilogue, one call that completes all frames (cw_signal rows are [C][F] of the call)
    rows, _, _, _, _ = run_fused(cfg, mcfg, iq, 4096, False, cw)
    # the stand-alone kernel on the same magnitudes
    m = U.Meter(channels, mcfg)
    alone = device_rows(channels, F)
    m.process_mag(torch.from_numpy(np.ascontiguousarray(om)).cuda(), torch.from_numpy(cw).cuda(), **alone)
    m.synchronize()
    alone = to_host(alone)
    for k in mc.OUTPUTS:
        assert mc.same(rows[k], want[k]).all(), ("fused", k, np.argwhere(~mc.same(rows[k], want[k]))[:3])
        assert mc.same(alone[k], want[k]).all(), ("meter_frames", k, np.argwhere(~mc.same(alone[k], want[k]))[:3])
    assert len(set(want["s_count"].ravel().tolist())) > 1
    if mode != "usb":
        assert len(set(want["snap_carrier_freq"].ravel().tolist())) > channels


def test_meter_reset(cuda):
    g = mc.load_case("sam_usb")
    m = U.Meter(g["channels"], mc.config_of(g))
    run_frames(g, m, 0, 5)
    m.reset()
    assert all((v == 0).all() for v in m.state().values())
    mc.check_rows(g, run_frames(g, m), what="after reset")


def test_attach_detach_and_refusals(cuda):
    import torch
    g = mc.load_case("p48_usb_256_usb")
    cfg = U.spectrum_config_from_ref_args(g["spec_args"])
    C, n = g["channels"], g["iq"].shape[1]
    d_iq = torch.from_numpy(g["iq"]).cuda()

    def spectrum_alone():
        spec = U.Spectrum(cfg, channels=C, frames=n)
        d_mag = torch.full(spec.out_shape, -1.0, dtype=torch.float32, device="cuda")
        d_avg = torch.full(spec.out_shape, -1.0, dtype=torch.float32, device="cuda")
        return spec, d_mag, d_avg

    spec, d_mag, d_avg = spectrum_alone()
    m = U.Meter(C, mc.config_of(g))
    rows = device_rows(C, spec.frames_out)
    spec.set_meter(m, **rows)
    assert spec.process(d_iq, d_mag, d_avg) == g["spec_frames"]
    torch.cuda.synchronize()
    mc.check_rows(g, to_host(rows), what="attached")
    before = m.state()
    # detached: the same call returns what a spectrum that never had a meter returns, and the meter stands still
    spec.set_meter(None)
    for v in rows.values():
        v.zero_()
    spec.reset()
    assert spec.process(d_iq, d_mag, d_avg) == g["spec_frames"]
    torch.cuda.synchronize()
    plain, p_mag, p_avg = spectrum_alone()
    plain.process(d_iq, p_mag, p_avg)
    torch.cuda.synchronize()
    assert_bitexact(d_mag.cpu().numpy(), p_mag.cpu().numpy(), "mag after detach")
    assert_bitexact(d_avg.cpu().numpy(), p_avg.cpu().numpy(), "avg after detach")
    assert_bitexact(d_mag.cpu().numpy(), g["mag"][:, :g["spec_frames"]], "mag after detach against the recording")
    assert all(bool((v == 0).all()) for v in rows.values())
    after = m.state()
    assert all(mc.same(before[k], after[k]).all() for k in mc.OUTPUTS)
    # refusals: another length, magnification or translation, a host meter, another channel count
    for bad in (dict(fft_len=512), dict(magnify=1), dict(iq_freq_mode=2)):
        other = U.Meter(C, U.meter_config(**bad))
        with pytest.raises(U.UhsdrError):
            spec.set_meter(other)
    with pytest.raises(U.UhsdrError):
        spec.set_meter(U.Meter(C, mc.config_of(g), host=True))
    with pytest.raises(U.UhsdrError):
        spec.set_meter(U.Meter(C + 1, mc.config_of(g)))
    s2 = torch.cuda.Stream()
    with pytest.raises(U.UhsdrError):
        spec.set_meter(U.Meter(C, mc.config_of(g), stream=s2.cuda_stream))
    spec.close()
    plain.close()


def test_attached_meter_moved_to_another_stream_is_refused(cuda):
    """the epilogue loads and stores the meter's state on the spectrum's stream: with the meter on
    another one a call is refused, and runs again once the meter is back"""
    import torch
    g = mc.load_case("p48_usb_256_usb")
    C, n = g["channels"], g["iq"].shape[1]
    spec = U.Spectrum(U.spectrum_config_from_ref_args(g["spec_args"]), channels=C, frames=n)
    m = U.Meter(C, mc.config_of(g))
    rows = device_rows(C, spec.frames_out)
    spec.set_meter(m, **rows)
    d_iq = torch.from_numpy(g["iq"]).cuda()
    other = torch.cuda.Stream()
    m.set_stream(other.cuda_stream)
    with pytest.raises(U.UhsdrError):
        spec.process(d_iq, None, None)
    torch.cuda.synchronize()
    assert untouched(rows)
    m.set_stream(0)
    assert spec.process(d_iq, None, None) == g["spec_frames"]
    torch.cuda.synchronize()
    mc.check_rows(g, to_host(rows), what="back on the stream")
    spec.close()
