"""The display stage's host side against the reference firmware's recordings (tests/display_cases.py):
the host twin of the frame (uhsdr_display_process_avg_host runs the step functions the kernels run),
the plan, the refusals, and the generated table header.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import display_cases as dc
import uhsdr_amd as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_host(g, d=None, first=0, frames=None):
    d = d or U.Display(g["channels"], dc.config_of(g), host=True)
    last = g["frames"] if frames is None else first + frames
    return d.process_avg_host(np.ascontiguousarray(g["avg"][:, first:last]), np.ascontiguousarray(g["edge"][:, first:last]))


def test_the_set_shows_what_it_must():
    assert len(dc.CASES) >= 31 and len(dc.SPEC_CASES) == 4
    dc.check_set()


@pytest.mark.parametrize("name", dc.CASES)
def test_host_twin_matches_reference_firmware(name):
    g = dc.load_case(name)
    dc.check_rows(g, run_host(g), what="host")


@pytest.mark.parametrize("name", dc.CASES)
def test_call_granularity(name):
    """F frames in one call equal F calls of one frame, and calls of three, with the state between them"""
    g = dc.load_case(name)
    for step in (1, 3):
        d = U.Display(g["channels"], dc.config_of(g), host=True)
        for first in range(0, g["frames"], step):
            n = min(step, g["frames"] - first)
            dc.check_rows(g, run_host(g, d, first, n), first=first, what=f"calls of {step}")
            st = d.state()
            assert dc.same(st["offset"], g["offset"][:, first + n - 1]).all() and dc.same(st["min"], g["min"][:, first + n - 1]).all()


@pytest.mark.parametrize("name", dc.CASES)
def test_plan_matches_the_firmwares_values(name):
    g = dc.load_case(name)
    p = U.display_plan(dc.config_of(g))
    got = np.array([p.db_scale, p.agc_rate, p.wfall_contrast], np.float32)
    assert dc.same(got, g["plan"]).all(), (got, g["plan"])
    assert (p.fft_len, p.width) == (g["L"], g["W"])
    assert p.reads_edge == int(g["reads_edge"])
    assert p.resample == int(g["W"] != g["L"])


def test_plan_of_the_default_configuration_and_the_panels():
    p = U.display_plan(U.display_config())
    assert (p.fft_len, p.width, p.resample, p.reads_edge, p.limit) == (256, 256, 0, 0, 20)
    assert p.agc_rate == 1.0 and p.wfall_contrast == np.float32(1.2) and p.db_scale == np.float32(31.6228)
    p = U.display_plan(U.display_config(fft_len=512))
    assert (p.width, p.resample, p.reads_edge, p.limit) == (480, 1, 1, 63)
    assert p.db_scale == np.float32(31.6228) * (np.float32(480) / np.float32(512))
    assert p.full_amount == np.float32(512) / np.float32(480)
    # the walk's last pixel: one whole sample, then the split at sample 512 with what is left of `amount`
    assert (p.first[479], p.whole[479]) == (511, 1) and 0 < p.amount[479] < 1e-4
    assert U.load().uhsdr_sizeof_display_config() == C.sizeof(U.DisplayConfig)
    assert U.load().uhsdr_sizeof_display_plan() == C.sizeof(U.DisplayPlan)


def test_the_walk_against_a_binary32_replay_of_the_firmwares_loop():
    """every accepted width of both lengths: first / whole / amount are what the loop of
    UiSpectrum_ScaleFFT2SpectrumWidth goes through, replayed here in binary32"""
    f32 = np.float32
    edges = 0
    for L in (256, 512):
        for W in range(L // 2, L):
            p = U.display_plan(U.display_config(fft_len=L, width=W))
            full = f32(L) / f32(W)
            amount, idx_old, reads = full, 0, False
            for x in range(W):
                first, n = idx_old, 0
                while amount >= 1:
                    idx_old += 1
                    n += 1
                    amount = f32(np.float64(amount) - 1.0)
                assert (p.first[x], p.whole[x]) == (first, n) and f32(p.amount[x]) == amount, (L, W, x)
                assert first >= x and idx_old <= L
                reads |= idx_old == L
                if x + 1 < W:
                    idx_old += 1
                    amount = full - (f32(1) - amount)
            assert p.reads_edge == int(reads), (L, W)
            edges += reads
    assert edges == 198             # of the 384 accepted pairs with W < L; two of them with a weight of exactly 0 (W = L / 2)


@pytest.mark.parametrize("bad", [
    dict(fft_len=1024), dict(fft_len=128), dict(fft_len=256, width=257), dict(fft_len=512, width=513), dict(fft_len=256, width=127),
    dict(fft_len=512, width=255), dict(spectrum_db_scale=-1), dict(spectrum_agc_rate=0), dict(spectrum_agc_rate=51),
    dict(waterfall_contrast=9), dict(waterfall_contrast=226), dict(scope_h=-1), dict(scope_h=65536),
], ids=str)
def test_refusals(bad):
    lib = U.load()
    cfg = U.display_config(**bad)
    plan = U.DisplayPlan()
    assert lib.uhsdr_display_plan_build(C.byref(cfg), C.byref(plan)) == U.UHSDR_ARGUMENT_ERROR
    assert b"display" in lib.uhsdr_last_error()
    h = C.c_void_p()
    assert lib.uhsdr_display_create_host(2, C.byref(cfg), C.byref(h)) == U.UHSDR_ARGUMENT_ERROR and not h.value


def test_wrong_kind_and_null_arguments():
    lib = U.load()
    d = U.Display(2, host=True)
    avg = np.ones((2, 1, 256), np.float32)
    assert lib.uhsdr_display_process_avg(d.handle, avg.ctypes.data_as(C.c_void_p), None, 1, None) == U.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_display_process_avg_host(d.handle, None, None, 1, None) == U.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_display_process_avg_host(d.handle, avg.ctypes.data_as(C.c_void_p), None, -1, None) == U.UHSDR_LENGTH_ERROR
    assert lib.uhsdr_display_set_stream(d.handle, None) == U.UHSDR_ARGUMENT_ERROR
    assert lib.uhsdr_display_create_host(0, C.byref(d.cfg), C.byref(C.c_void_p())) == U.UHSDR_ARGUMENT_ERROR
    with pytest.raises(ValueError):
        d.process_avg(avg)
    with pytest.raises(ValueError):
        d.process_avg_host(np.ones((2, 1, 512), np.float32))


def test_state_reset_and_null_rows():
    g = dc.load_case("step")
    d = U.Display(g["channels"], dc.config_of(g), host=True)
    st = d.state()
    assert (st["offset"] == -80).all() and (st["min"] == 0).all()
    run_host(g, d, 0, 4)
    # a null io and a null edge row still move the state (the offset does not depend on the edge)
    rest = np.ascontiguousarray(g["avg"][:, 4:])
    d._call("process_avg_host", rest.ctypes.data_as(C.c_void_p), None, rest.shape[1], None)
    assert dc.same(d.state()["offset"], g["offset"][:, -1]).all() and dc.same(d.state()["min"], g["min"][:, -1]).all()
    d.reset()
    assert (d.state()["offset"] == -80).all() and (d.state()["min"] == 0).all()
    dc.check_rows(g, run_host(g, d), what="after reset")


def test_null_edge_is_zero_and_an_unread_edge_is_ignored():
    g = dc.load_case("edge_1e6")
    got = U.Display(g["channels"], dc.config_of(g), host=True).process_avg_host(g["avg"])
    zero = U.Display(g["channels"], dc.config_of(g), host=True).process_avg_host(g["avg"], np.zeros_like(g["edge"]))
    assert all(dc.same(got[k], zero[k]).all() for k in dc.OUTPUTS)
    assert (got["scope"][:, :, -1] != g["scope"][:, :, -1]).all() and (got["scope"][:, :, :-1] == g["scope"][:, :, :-1]).all()
    g = dc.load_case("w256_200")
    wild = U.Display(g["channels"], dc.config_of(g), host=True).process_avg_host(g["avg"], np.full_like(g["edge"], 1e30))
    dc.check_rows(g, wild, what="edge 1e30 where the walk does not read it")


def test_factor_zero_makes_every_sig_the_offset():
    """spectrum_db_scale 0 has factor 0: the minimum is the offset itself and the AGC is a plain binary32 recursion"""
    cfg = U.display_config(spectrum_db_scale=0, spectrum_agc_rate=25)
    d = U.Display(1, cfg, host=True)
    got = d.process_avg_host(np.ones((1, 3, 256), np.float32))
    # agc_rate 1: offset -= min / 5 with min == offset, all binary32
    o = np.float32(-80)
    for f in range(3):
        assert got["min"][0, f] == o
        o = np.float32(o - np.float32(np.float32(1) * o) / np.float32(5))
        assert got["offset"][0, f] == o


def test_table_header_is_what_the_fixture_gives():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "display", "gen_display_tables.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
