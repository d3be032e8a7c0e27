"""The display stage on the device against the reference firmware's recordings (tests/display_cases.py):
the stand-alone kernel display_frames on every case, the stage as the spectrum kernel's epilogue on
the cases recorded from I/Q (driven from that I/Q, at call sizes that complete none, one and four
frames, with and without mag / avg, with and without a meter attached), ragged batches against the
host twin, reset, and attach / detach.  Bit for bit on all four outputs."""
import os

import numpy as np
import pytest

import display_cases as dc
import meter_cases as mc
import oracle
import uhsdr_amd as U
from golden_util import assert_bitexact
from uhsdr_amd import display, meter, synth

pytestmark = pytest.mark.gpu

SENTINEL = -7           # what a row holds before a call (249 in a byte): no output of any case but the negative one
IQ_CASES = dc.SPEC_CASES + [dc.NYQUIST]


def device_rows(d, F):
    """the four rows as tensors (the uint16 row as int16: the same two bytes), filled with SENTINEL"""
    import torch
    kinds = {np.uint16: torch.int16, np.uint8: torch.uint8, np.float32: torch.float32}
    return {name: torch.full(d.row_shape(name, F), SENTINEL % 256 if dt is np.uint8 else SENTINEL, dtype=kinds[dt], device="cuda")
            for name, dt in display.OUTPUTS}


def to_host(rows, n=None):
    types = dict(display.OUTPUTS)
    return {k: np.ascontiguousarray(v.cpu().numpy()[:, :n]).view(types[k]) for k, v in rows.items()}


def untouched(rows):
    return all(bool((v == (SENTINEL % 256 if v.element_size() == 1 else SENTINEL)).all()) for v in rows.values())


def meter_rows(C, F):
    """the meter's six rows as tensors (the uint32 row as int32), filled with SENTINEL"""
    import torch
    return {name: torch.full((C, F), SENTINEL, dtype=torch.float32 if dt is np.float32 else torch.int32, device="cuda")
            for name, dt in meter.OUTPUTS}


def meter_to_host(rows, n=None):
    types = dict(meter.OUTPUTS)
    return {k: np.ascontiguousarray(v.cpu().numpy()[:, :n]).view(types[k]) for k, v in rows.items()}


def run_frames(g, d=None, first=0, frames=None):
    import torch
    d = d or U.Display(g["channels"], dc.config_of(g))
    last = g["frames"] if frames is None else first + frames
    rows = device_rows(d, last - first)
    d.process_avg(torch.from_numpy(np.ascontiguousarray(g["avg"][:, first:last])).cuda(),
                  torch.from_numpy(np.ascontiguousarray(g["edge"][:, first:last])).cuda(), **rows)
    d.synchronize()
    return to_host(rows)


@pytest.mark.parametrize("name", dc.CASES)
def test_display_frames_matches_reference_firmware(cuda, name):
    g = dc.load_case(name)
    dc.check_rows(g, run_frames(g), what="display_frames")


def test_display_frames_call_granularity_state_and_reset(cuda):
    g = dc.load_case("step")
    d = U.Display(g["channels"], dc.config_of(g))
    for first in range(0, g["frames"], 5):
        n = min(5, g["frames"] - first)
        dc.check_rows(g, run_frames(g, d, first, n), first=first, what="calls of 5")
    st = d.state()
    assert dc.same(st["offset"], g["offset"][:, -1]).all() and dc.same(st["min"], g["min"][:, -1]).all()
    d.reset()
    assert (d.state()["offset"] == -80).all() and (d.state()["min"] == 0).all()
    dc.check_rows(g, run_frames(g, d), what="after reset")


def test_null_edge_and_null_rows(cuda):
    import torch
    g = dc.load_case("edge_1e6")
    d = U.Display(g["channels"], dc.config_of(g))
    rows = device_rows(d, g["frames"])
    d.process_avg(torch.from_numpy(g["avg"]).cuda(), None, scope=rows["scope"])
    d.synchronize()
    want = U.Display(g["channels"], dc.config_of(g), host=True).process_avg_host(g["avg"])
    assert (to_host(rows)["scope"] == want["scope"]).all()
    assert untouched({k: v for k, v in rows.items() if k != "scope"})
    assert dc.same(d.state()["offset"], g["offset"][:, -1]).all()


def run_fused(cfg, dcfg, iq, per_call, want_spec, mcfg=None):
    """the spectrum with a display (and a meter) attached over iq [C][n][2] in calls of per_call input
    frames: the display's rows, the meter's, mag and avg of every completed frame; a call that completes
    nothing must write nothing"""
    import torch
    C, n, _ = iq.shape
    spec = U.Spectrum(cfg, channels=C, frames=per_call)
    d = U.Display(C, dcfg)
    F = spec.frames_out
    rows = device_rows(d, F)
    spec.set_display(d, **rows)
    m, mrows = None, {}
    if mcfg is not None:
        m = U.Meter(C, mcfg)
        mrows = meter_rows(C, F)
        spec.set_meter(m, **mrows)
    d_mag = torch.full(spec.out_shape, -1.0, dtype=torch.float32, device="cuda") if want_spec else None
    d_avg = torch.full(spec.out_shape, -1.0, dtype=torch.float32, device="cuda") if want_spec else None
    d_iq = torch.empty((C, per_call, 2), dtype=torch.int32, device="cuda")
    out, mout = {k: [] for k in dc.OUTPUTS}, {k: [] for k in mc.OUTPUTS}
    mags, avgs, idle = [], [], 0
    for off in range(0, n, per_call):
        d_iq.copy_(torch.from_numpy(np.ascontiguousarray(iq[:, off:off + per_call])))
        nf = spec.process(d_iq, d_mag, d_avg)
        torch.cuda.synchronize()
        if nf == 0:
            idle += 1
            if idle <= 3:           # reading all rows back after each of hundreds of calls would only slow the test
                assert untouched(rows) and untouched(mrows), f"a call that completed no frame wrote (input frame {off})"
            continue
        for k, v in to_host(rows, nf).items():
            out[k].append(v)
        if mrows:
            for k, v in meter_to_host(mrows, nf).items():
                mout[k].append(v)
        if want_spec:
            mags.append(d_mag[:, :nf].cpu().numpy())
            avgs.append(d_avg[:, :nf].cpu().numpy())
        for v in list(rows.values()) + list(mrows.values()):
            v.fill_(SENTINEL % 256 if v.element_size() == 1 else SENTINEL)
    state = d.state()
    spec.close()
    d.close()
    if m:
        m.close()
    cat = lambda xs: np.concatenate(xs, axis=1) if xs else None  # noqa: E731
    return {k: cat(v) for k, v in out.items()}, {k: cat(v) for k, v in mout.items()}, cat(mags), cat(avgs), state, idle


def case_iq(g):
    return g["iq"], U.spectrum_config_from_ref_args(g["spec_args"]), 1 << g["spec_args"].get("mag", 0)


@pytest.mark.parametrize("size,want_spec,metered", [("none", False, True), ("one", True, False), ("four", False, False), ("four", True, True)])
@pytest.mark.parametrize("name", IQ_CASES)
def test_fused_display_matches_reference_firmware(cuda, name, size, want_spec, metered):
    g = dc.load_case(name)
    iq, cfg, zd = case_iq(g)
    per_call = {"none": 32, "one": g["L"] * zd, "four": 4 * g["L"] * zd}[size]
    # the meter of the same source as tests/golden/meter_<source>_usb.npz has it, where there is one
    mg = mc.load_case(f"{name}_usb") if metered and f"{name}_usb" in mc.CASES else None
    mcfg = None
    if metered:
        mcfg = mc.config_of(mg) if mg else U.meter_config(fft_len=g["L"], magnify=g["spec_args"].get("mag", 0))
    rows, mrows, mag, avg, state, idle = run_fused(cfg, dc.config_of(g), iq, per_call, want_spec, mcfg)
    n = g["frames"]
    assert rows["offset"].shape == (g["channels"], n)
    dc.check_rows(g, rows, frames=n, what=f"fused, calls of {per_call}")
    assert dc.same(state["offset"], g["offset"][:, -1]).all() and dc.same(state["min"], g["min"][:, -1]).all()
    if size == "none":
        assert idle > 0             # the accumulate path ran
    if want_spec:
        assert_bitexact(avg, g["avg"], "FFT_AVGData beside the display")
        if g["spec"]:
            with np.load(os.path.join(dc.GOLDEN, f"spec_{g['spec']}.npz")) as z:
                assert_bitexact(mag, z["mag"], "FFT_MagData beside the display")
    if mg:
        mc.check_rows(mg, mrows, frames=n, what="the meter beside the display")
    elif metered:
        # no meter recording of this source: the meter's host twin on the magnitudes of a spectrum call of its own
        if mag is None:
            mag = run_fused(cfg, dc.config_of(g), iq, 4 * g["L"] * zd, True)[2]
        want = U.Meter(g["channels"], mcfg, host=True).process_mag_host(np.ascontiguousarray(mag))
        for k in mc.OUTPUTS:
            assert mc.same(mrows[k], want[k]).all(), k


@pytest.mark.parametrize("L,width,channels", [(256, 0, 5), (512, 511, 9), (512, 0, 9), (256, 200, 9)])
def test_ragged_batches_match_host_twin(cuda, L, width, channels):
    """one full workgroup of four waves plus a partial one, every channel at another level: the fused
    call and display_frames against the host twin on the average the same call wrote.  The host twin
    gets no edge (the call does not hand it out): at 512 -> 480, where the walk reads it, the last
    column is left to the recorded cases and everything else is compared."""
    import torch
    cfg = U.default_spectrum_config(fft_len=L, spectrum_filter=3, iq_gain_i=1.01, iq_gain_q=0.99, iq_phase_balance=-0.003)
    dcfg = U.display_config(fft_len=L, width=width, spectrum_agc_rate=10)
    iq = synth.ssb_iq(np.arange(channels), 7, 4096)
    iq = np.ascontiguousarray((iq.astype(np.float64) * (0.05 + 0.95 * np.arange(channels) / channels)[:, None, None]).astype(np.int32))
    rows, _, _, avg, state, _ = run_fused(cfg, dcfg, iq, 4096, True)
    om, oa = oracle.OracleSpectrum(U.build_spectrum_plan(cfg), channels).process(iq, threads=8)
    assert_bitexact(avg, oa, "the average beside the display against the CPU oracle")
    host = U.Display(channels, dcfg, host=True)
    want = host.process_avg_host(np.ascontiguousarray(avg))
    d = U.Display(channels, dcfg)
    alone = device_rows(d, avg.shape[1])
    d.process_avg(torch.from_numpy(np.ascontiguousarray(avg)).cuda(), None, **alone)
    d.synchronize()
    alone = to_host(alone)
    cols = slice(None, -1) if host.plan.reads_edge else slice(None)
    for k in dc.OUTPUTS:
        a, b, w = (x[k][..., cols] if k in display.WIDE else x[k] for x in (rows, alone, want))
        assert dc.same(a, w).all(), ("fused", k, np.argwhere(~dc.same(a, w))[:3])
        assert dc.same(b, w).all(), ("display_frames", k, np.argwhere(~dc.same(b, w))[:3])
    assert dc.same(alone["scope"], want["scope"]).all() and dc.same(alone["wfall"], want["wfall"]).all()
    assert dc.same(state["offset"], want["offset"][:, -1]).all()
    assert len(set(want["offset"][:, -1].tolist())) == channels       # no two channels share a state


def test_attach_detach_and_refusals(cuda):
    import torch
    g = dc.load_case("p48_usb_512")
    iq, cfg, _ = case_iq(g)
    C, n = g["channels"], iq.shape[1]
    d_iq = torch.from_numpy(iq).cuda()

    def spectrum_alone():
        spec = U.Spectrum(cfg, channels=C, frames=n)
        d_mag = torch.full(spec.out_shape, -1.0, dtype=torch.float32, device="cuda")
        d_avg = torch.full(spec.out_shape, -1.0, dtype=torch.float32, device="cuda")
        return spec, d_mag, d_avg

    spec, d_mag, d_avg = spectrum_alone()
    d = U.Display(C, dc.config_of(g))
    rows = device_rows(d, spec.frames_out)
    spec.set_display(d, **rows)
    assert spec.process(d_iq, d_mag, d_avg) == g["frames"]
    torch.cuda.synchronize()
    dc.check_rows(g, to_host(rows), what="attached")
    before = d.state()
    # detached: the same call returns what a spectrum that never had a display returns, and the display stands still
    spec.set_display(None)
    for v in rows.values():
        v.fill_(SENTINEL % 256 if v.element_size() == 1 else SENTINEL)
    spec.reset()
    assert spec.process(d_iq, d_mag, d_avg) == g["frames"]
    torch.cuda.synchronize()
    plain, p_mag, p_avg = spectrum_alone()
    plain.process(d_iq, p_mag, p_avg)
    torch.cuda.synchronize()
    assert_bitexact(d_mag.cpu().numpy(), p_mag.cpu().numpy(), "mag after detach")
    assert_bitexact(d_avg.cpu().numpy(), p_avg.cpu().numpy(), "avg after detach")
    assert_bitexact(d_avg.cpu().numpy(), g["avg"], "avg after detach against the recording")
    assert untouched(rows)
    after = d.state()
    assert all(dc.same(before[k], after[k]).all() for k in ("offset", "min"))
    # refusals: another length, a host display, another channel count, another stream
    with pytest.raises(U.UhsdrError):
        spec.set_display(U.Display(C, U.display_config(fft_len=256)))
    with pytest.raises(U.UhsdrError):
        spec.set_display(U.Display(C, dc.config_of(g), host=True))
    with pytest.raises(U.UhsdrError):
        spec.set_display(U.Display(C + 1, dc.config_of(g)))
    s2 = torch.cuda.Stream()
    with pytest.raises(U.UhsdrError):
        spec.set_display(U.Display(C, dc.config_of(g), stream=s2.cuda_stream))
    # moved to another stream while attached: the call is refused and writes nothing, and runs again once it is back
    spec.set_display(d, **rows)
    d.set_stream(s2.cuda_stream)
    with pytest.raises(U.UhsdrError):
        spec.process(d_iq, None, None)
    torch.cuda.synchronize()
    assert untouched(rows)
    d.set_stream(0)
    d.reset()
    spec.reset()
    assert spec.process(d_iq, None, None) == g["frames"]
    torch.cuda.synchronize()
    dc.check_rows(g, to_host(rows), what="back on the stream")
    spec.close()
    plain.close()
