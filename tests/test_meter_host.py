"""The signal meter's host side against the reference firmware's recordings (tests/meter_cases.py):
the host twin of the frame (uhsdr_meter_process_mag_host runs the step functions the kernels run),
the plan, the refusals, and the generated table header.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import meter_cases as mc
import uhsdr_amd as U
from uhsdr_amd import _abi, meter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_host(g, m=None, first=0, frames=None):
    m = m or U.Meter(g["channels"], mc.config_of(g), host=True)
    last = g["frames"] if frames is None else first + frames
    return m.process_mag_host(np.ascontiguousarray(g["mag"][:, first:last]), np.ascontiguousarray(g["cw_signal"][:, first:last]))


def test_the_set_shows_what_it_must():
    assert len(mc.CASES) >= 42 and len(mc.SPEC_CASES) == 12
    mc.check_set()


@pytest.mark.parametrize("name", mc.CASES)
def test_host_twin_matches_reference_firmware(name):
    g = mc.load_case(name)
    mc.check_rows(g, run_host(g), what="host")


@pytest.mark.parametrize("name", mc.CASES)
def test_plan_matches_the_firmwares_bins(name):
    g = mc.load_case(name)
    p = U.meter_plan(mc.config_of(g))
    assert [p.lbin, p.ubin, p.posbin] == g["bins"].tolist()
    assert p.snap == g["snap_mode"]
    assert p.fft_len == g["L"]


def test_passband_of_one_bin():
    """Lbin == Ubin through the firmware's own clamp: 300 Hz at 900 Hz on the lower sideband, magnify 5.
    The dBm/Hz term is ten times the fast logarithm of 0, a finite number, and the recording has it."""
    g = mc.load_case("cw_onebin")
    assert g["bins"].tolist() == [0, 0, 128]
    assert np.isfinite(g["dbmhz_cur"]).all() and not (g["dbmhz_cur"] == g["dbm_cur"]).any()
    for L in (256, 512):
        p = U.meter_plan(U.meter_config(**dict(g["cfg"], fft_len=L)))
        assert (p.lbin, p.ubin) == (0, 0) and np.isfinite(p.dbmhz_term) and p.dbmhz_term < 0
    term = U.meter_plan(mc.config_of(g)).dbmhz_term
    assert mc.same(g["dbmhz_cur"], (g["dbm_cur"] - np.float32(term)).astype(np.float32)).all()


def test_plan_of_the_default_configuration():
    p = U.meter_plan(U.meter_config())
    # 256 bins of 187.5 Hz, LO 12 kHz below: the carrier 64 bins above the centre; 3.8 kHz of USB above it
    assert (p.bin_bw, p.bin_offset, p.posbin, p.lbin, p.ubin) == (187.5, 64, 192, 192, 212)
    assert (p.width, p.offset, p.bw_lower, p.bw_upper) == (3800.0, 1900.0, 0.0, 3800.0)
    assert p.cons == -225.0 and p.snap == 0 and p.snap_offset == 0.0
    assert p.attack_alpha == np.float32(50) * np.float32(0.01) and p.decay_alpha == np.float32(5) * np.float32(0.01)
    assert U.meter_plan(U.meter_config(fft_len=512)).cons == -228.0
    assert list(p.s_cal_dbm)[:2] == [-124.0, -121.0] and p.s_cal_dbm[32] == 2.0
    assert U.load().uhsdr_sizeof_meter_config() == C.sizeof(U.MeterConfig)
    assert U.load().uhsdr_sizeof_meter_plan() == C.sizeof(U.MeterPlan)


def test_snap_modes_and_offsets():
    cw = U.meter_plan(U.meter_config(dmod_mode=U.DEMOD_CW, filter_path=9, cw_sidetone_freq=700))
    assert (cw.snap, cw.snap_offset) == (2, -700.0)
    assert U.meter_plan(U.meter_config(dmod_mode=U.DEMOD_CW, filter_path=9, cw_lsb=1)).snap_offset == 750.0
    psk = dict(dmod_mode=U.DEMOD_DIGI, digital_mode=U.DIGITAL_MODE_BPSK)
    assert U.meter_plan(U.meter_config(**psk)).snap_offset == -500.0
    assert U.meter_plan(U.meter_config(digi_lsb=1, **psk)).snap_offset == 500.0
    assert U.meter_plan(U.meter_config(dmod_mode=U.DEMOD_DIGI, digital_mode=U.DIGITAL_MODE_RTTY)).snap == 0
    assert U.meter_plan(U.meter_config(dmod_mode=U.DEMOD_AM, filter_path=2)).snap == 1
    assert U.meter_plan(U.meter_config(dmod_mode=U.DEMOD_AM, filter_path=2, snap_enable=0)).snap == 0


@pytest.mark.parametrize("bad", [
    dict(fft_len=1024), dict(fft_len=128), dict(magnify=6), dict(magnify=-1), dict(iq_freq_mode=5), dict(dmod_mode=9),
    dict(filter_path=0), dict(filter_path=87), dict(sam_sideband=4), dict(dbm_constant=101), dict(dbm_constant=-101),
    dict(attack_alpha=0), dict(decay_alpha=101),
    # a 300 Hz CW filter centred on 950 Hz at magnify 5: Lbin 265 lies past the last bin, Ubin is clamped to 255
    dict(dmod_mode=2, filter_path=13, magnify=5),
    # the same below the first bin on the lower sideband: Ubin -9 with Lbin clamped to 0
    dict(dmod_mode=2, filter_path=13, magnify=5, cw_lsb=1),
], ids=str)
def test_refusals(bad):
    lib = U.load()
    cfg = U.meter_config(**bad)
    plan = U.MeterPlan()
    assert lib.uhsdr_meter_plan_build(C.byref(cfg), C.byref(plan)) == U.UHSDR_ARGUMENT_ERROR
    assert b"meter" in lib.uhsdr_last_error()
    h = C.c_void_p()
    assert lib.uhsdr_meter_create_host(2, C.byref(cfg), C.byref(h)) == U.UHSDR_ARGUMENT_ERROR and not h.value


def test_wrong_kind_and_null_arguments():
    lib = U.load()
    m = U.Meter(2, host=True)
    mag = np.zeros((2, 1, 256), np.float32)
    assert lib.uhsdr_meter_process_mag(m.handle, mag.ctypes.data_as(C.c_void_p), 1, None) == U.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_meter_process_mag_host(m.handle, None, 1, None) == U.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_meter_process_mag_host(m.handle, mag.ctypes.data_as(C.c_void_p), -1, None) == U.UHSDR_LENGTH_ERROR
    assert lib.uhsdr_meter_set_stream(m.handle, None) == U.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_meter_create_host(0, C.byref(m.cfg), C.byref(C.c_void_p())) == U.UHSDR_ARGUMENT_ERROR
    with pytest.raises(ValueError):
        m.process_mag(mag)
    with pytest.raises(ValueError):
        m.process_mag_host(np.zeros((2, 1, 512), np.float32))


@pytest.mark.parametrize("name", ["p48_usb_256_lsb", "cw300_p4_usb", "cw_onebin", "sam_usb", "step", "nan"])
def test_call_granularity(name):
    """F frames in one call equal F calls of one frame, and any other split"""
    g = mc.load_case(name)
    for step in (1, 3):
        m = U.Meter(g["channels"], mc.config_of(g), host=True)
        for first in range(0, g["frames"], step):
            n = min(step, g["frames"] - first)
            mc.check_rows(g, run_host(g, m, first, n), first=first, what=f"calls of {step}")


def test_state_and_reset():
    g = mc.load_case("am")
    m = U.Meter(g["channels"], mc.config_of(g), host=True)
    st = m.state()
    assert all((st[k] == 0).all() for k in mc.OUTPUTS)
    run_host(g, m, 0, 4)
    st = m.state()
    for k in mc.OUTPUTS:
        assert mc.same(st[k], g[k][:, 3]).all(), k
    # a null io still moves the state
    half = np.ascontiguousarray(g["mag"][:, 4:])
    m._call("process_mag_host", half.ctypes.data_as(C.c_void_p), half.shape[1], None)
    for k in mc.OUTPUTS:
        assert mc.same(m.state()[k], g[k][:, -1]).all(), k
    m.reset()
    assert all((m.state()[k] == 0).all() for k in mc.OUTPUTS)
    mc.check_rows(g, run_host(g, m), what="after reset")      # freq_old is 1e7 again


def test_maximum_in_the_last_bin_reads_zero_behind_it():
    """The library's own definition, not the firmware's: with maxbin == L - 1 the firmware reads
    sd.FFT_Samples[L]; here bin3 is 0.  AM at magnify 5 has the passband [0, 255]."""
    cfg = U.meter_config(dmod_mode=U.DEMOD_AM, filter_path=2, magnify=5, tune_old=7100000)
    p = U.meter_plan(cfg)
    assert (p.lbin, p.ubin, p.posbin) == (0, 255, 128)
    L = 256
    mag = np.full((1, 1, L), 2.0, np.float32)
    mag[0, 0, mc.sample_index(L, 255)] = 900.0
    mag[0, 0, mc.sample_index(L, 254)] = 300.0
    got = U.Meter(1, cfg, host=True).process_mag_host(mag)["snap_carrier_freq"][0, 0]
    f32, bw = np.float32, np.float64(p.bin_bw)
    bin1, bin2, bin3 = f32(300.0) * f32(1000), f32(900.0) * f32(1000), f32(0)
    delta1 = f32((np.float64(255) + 1.0 - np.float64(128)) * bw)
    delta2 = f32(bw * (1.36 * np.float64(bin3 - bin1)) / np.float64(f32(bin1 + bin2) + bin3))
    help_freq = f32(f32(7100000) + f32(delta1 + delta2))
    assert got == int(f32(0.2 * np.float64(help_freq) + 0.8 * 1e7))
    # and it is the neighbour that is defined away, not the search: the same carrier one bin lower reads its real neighbour
    mag2 = np.full((1, 1, L), 2.0, np.float32)
    mag2[0, 0, mc.sample_index(L, 254)] = 900.0
    mag2[0, 0, mc.sample_index(L, 253)] = 300.0
    assert U.Meter(1, cfg, host=True).process_mag_host(mag2)["snap_carrier_freq"][0, 0] != got


def test_table_header_is_what_the_fixture_gives():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "meter", "gen_meter_tables.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
