"""rx_front over the shapes its host code chooses between: every kernel family at 8 and at 16 FIR
outputs per lane (uhsdr_rx_set_front_block), call sizes that are no power of two (lanes per channel
nb = N / R = 12, 20, 24, 40; 6, 10, 20 at R = 16: channels per wave cpw = 64 / nb = 5, 3, 2, 1; 10,
6, 3, with idle lanes, front_lane's g = l / nb map and front waves that straddle two back-end
groups), one to three launches per call, the block changed between calls in the serial mode and
under every hand-off of uhsdr_rx_set_pipelined, the call sizes rx_chain takes or refuses, and
refused blocks that must leave the handle as it was.

Every comparison is bit-exact against the CPU oracle on the same synthetic input (audio with
assert_bitexact, the codec frames with assert_array_equal), except the FMA cases, which are held
to the project's 1e-5 normwise bound (tests/test_gpu_fma.py).  The oracle runs once per
(family, channel count): it works in 32-frame calls whatever the device's call size, so every
shape compares against a prefix of the same read-only reference.  No case compares silence: the
reference's last call must be non-zero, and FM runs past the squelch's opening (200 32-frame calls).

C = 67 is two back-end groups with a partial last front wave for every cpw above; the hand-off
cases use C = 130 (three groups, the last of two channels).
"""
import functools

import numpy as np
import pytest

import oracle
import uhsdr_amd as U
from golden_util import assert_bitexact
from test_gpu_fma import TOL, normwise
from test_gpu_parity import DeviceStream, run_device
from test_gpu_pipelined import run_pipelined
from uhsdr_amd import synth

pytestmark = pytest.mark.gpu

# one configuration per rx_front family (uhsdr_rx_variants.inc kFront), AM and SAM both on P70
FAMILIES = {
    "wide_p48_usb": (dict(filter_path=48, dmod_mode=U.DEMOD_USB), synth.ssb_iq),
    "24k_p60_usb": (dict(filter_path=60, dmod_mode=U.DEMOD_USB), synth.ssb_iq),
    "narrow_p35_lsb": (dict(filter_path=35, dmod_mode=U.DEMOD_LSB), functools.partial(synth.ssb_iq, lsb=True)),
    "narrow_p4_cw": (dict(filter_path=4, dmod_mode=U.DEMOD_CW), synth.cw_iq),
    "am_p70": (dict(filter_path=70, dmod_mode=U.DEMOD_AM), synth.am_iq),
    "sam_p70": (dict(filter_path=70, dmod_mode=U.DEMOD_SAM), synth.am_iq),
    "am24k_p83": (dict(filter_path=83, dmod_mode=U.DEMOD_AM), synth.am_iq),
    "fm_p1": (dict(filter_path=1, dmod_mode=U.DEMOD_FM, fm_sql_threshold=0), synth.fm_iq),
    "st_wide_p48": (dict(filter_path=48, dmod_mode=U.DEMOD_SSBSTEREO, stereo_enable=1), synth.ssb_iq),
    "st_24k_p55_iq": (dict(filter_path=55, dmod_mode=U.DEMOD_IQ, stereo_enable=1), synth.ssb_iq),
    "st_narrow_p35": (dict(filter_path=35, dmod_mode=U.DEMOD_SSBSTEREO, stereo_enable=1), synth.ssb_iq),
}

FM_FRAMES = 7168        # 224 32-frame calls: the squelch's first decision (call 200) is inside
REF_FRAMES = 9216       # the longest case: the FM switch case, 36 calls of 256 frames


def is_fm(name):
    return FAMILIES[name][0]["dmod_mode"] == U.DEMOD_FM


@functools.lru_cache(maxsize=None)
def reference(name, C):
    """(cfg, iq, a_buffer[1], a_buffer[0], dst) of REF_FRAMES frames (FM), or 8192 (the others'
    longest case: 8 calls of 1024); computed once, read-only"""
    kw, gen = FAMILIES[name]
    cfg = U.default_config(**kw)
    iq = gen(np.arange(C), 0, REF_FRAMES if is_fm(name) else 8192)
    r1, r0, rdst = oracle.OracleRx(U.build_plan(cfg), C).process2(iq, threads=8)
    for a in (iq, r1, r0, rdst):
        a.setflags(write=False)
    return cfg, iq, r1, r0, rdst


def calls_for(name, N):
    """at least 4 calls; past the AGC's 6-call ring where the call is 64 frames or shorter; FM: past
    the squelch's opening"""
    calls = 4 if N > 64 else 8
    if is_fm(name):
        calls = max(calls, -(-FM_FRAMES // N))
    return calls


def check_audible(name, ref, n, N):
    assert np.abs(ref[:, n - N:n]).max() > 0, f"{name}: the reference's last call is silent"
    if is_fm(name):
        assert (np.abs(ref[:, n - 2048:n]).max(axis=1) > 0).all(), f"{name}: FM squelch still closed"


def set_block(R):
    """run_device hook: R outputs per lane from the first call on (strict: raises if not available)"""
    def hook(chain, k):
        if k == 0 and R != 8:
            chain.set_front_block(R)
    return hook


def switch_blocks(blocks):
    def hook(chain, k):
        if k in blocks:
            chain.set_front_block(blocks[k])
    return hook


def run_family(name, C, N, n, hook):
    """-> got (a1, a0 or None, dst), ref (a1, a0 or None, dst) over n frames in N-frame calls"""
    cfg, iq, r1, r0, rdst = reference(name, C)
    assert n <= iq.shape[1]
    stereo = bool(FAMILIES[name][0].get("stereo_enable"))
    if stereo:
        assert U.build_plan(cfg).stereo
        dev = DeviceStream(cfg, C, N)
        outs = []
        for k in range(n // N):
            hook(dev.chain, k)
            outs.append(dev(np.ascontiguousarray(iq[:, k * N:(k + 1) * N])))
        dev.chain.close()
        a1, a0, dst = (np.concatenate([o[i] for o in outs], axis=1) for i in range(3))
    else:
        a1, dst = run_device(cfg, iq[:, :n], N, hook=hook)
        a0 = None
    return (a1, a0, dst), (r1[:, :n], r0[:, :n] if stereo else None, rdst[:, :n])


def assert_family_exact(name, got, ref, what):
    assert_bitexact(got[0], ref[0], f"{name} {what} a_buffer[1]")
    if got[1] is not None:
        assert_bitexact(got[1], ref[1], f"{name} {what} a_buffer[0]")
    np.testing.assert_array_equal(got[2], ref[2])


# R = 8: cpw 5, 3, 2, 1 and three launches per call; R = 16: cpw 16, 10, 6, 3, 2 and one launch
# where R = 8 takes two
SHAPES = [(8, N) for N in (96, 160, 192, 320, 1536)] + [(16, N) for N in (64, 96, 160, 320, 512, 1024)]


@pytest.mark.parametrize("R,N", SHAPES, ids=[f"R{R}-N{N}" for R, N in SHAPES])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_front_block_and_call_size_match_oracle(cuda, name, R, N):
    """Every front family at both block sizes and at call sizes that are no power of two, the
    wave pipeline behind it (the back ends read adec the same way for every front shape)."""
    C = 67
    n = calls_for(name, N) * N
    got, ref = run_family(name, C, N, n, set_block(R))
    assert_family_exact(name, got, ref, f"R={R} N={N}")
    check_audible(name, ref[0], n, N)


FMA_FAMILIES = ["wide_p48_usb", "fm_p1", "st_wide_p48"]


@pytest.mark.parametrize("N", [96, 256])
@pytest.mark.parametrize("name", FMA_FAMILIES)
def test_front_block_fma(cuda, name, N):
    """The fn_fma kernels at 16 outputs per lane, on the families that accept FMA: within 1e-5
    normwise per channel of the oracle (the one comparison here that is not bit-exact), and not the
    EXACT bits (FM aside: the discriminator's atan2 of a ratio absorbs the FIR's last-bit differences).
    Measured on an MI355X (normwise maximum over 67 channels): P48 USB 3.3e-6 (N = 96) / 4.0e-6
    (256), FM P1 1.2e-6 / 1.2e-6, stereo P48 3.3e-6 / 4.0e-6 (a_buffer[1]) and 2.0e-6 / 2.0e-6
    (a_buffer[0]): inside the acceptance table's figures for 8 outputs per lane (uhsdr_rx_plan_fma_ok)."""
    C = 67
    n = max(calls_for(name, N), 8) * N

    def hook(chain, k):
        if k == 0:
            chain.set_front_block(16)
            chain.set_precision(U.PRECISION_FMA)
            assert chain.precision == U.PRECISION_FMA

    got, ref = run_family(name, C, N, n, hook)
    check_audible(name, ref[0], n, N)
    for g, r, what in ((got[0], ref[0], "a_buffer[1]"), (got[1], ref[1], "a_buffer[0]")):
        if g is None:
            continue
        assert np.isfinite(g).all()
        err = normwise(g, r)
        print(f"{name} N={N} R=16 FMA {what}: normwise max {err.max():.3g} median {np.median(err):.3g}")
        assert err.max() <= TOL, f"{name} N={N} {what}: normwise error {err.max():.3g} > {TOL}"
        if not is_fm(name):
            assert not np.array_equal(g.view(np.uint32), r.view(np.uint32)), f"{name} {what}: FMA output is bit-exact"


# (family, N, calls before the switching stretch): P35's pass-1 window is padded at R = 8 only, so
# the history rows in HBM must mean the same under both; P70 SAM at 1024 goes from two launches per
# call to one; FM starts after the squelch has opened
SWITCH_SERIAL = [("wide_p48_usb", 256, 0), ("narrow_p35_lsb", 256, 0), ("sam_p70", 1024, 0), ("fm_p1", 256, 28)]


@pytest.mark.parametrize("name,N,lead", SWITCH_SERIAL, ids=[f"{c[0]}-N{c[1]}" for c in SWITCH_SERIAL])
def test_front_block_switch_serial(cuda, name, N, lead):
    """One handle, serial mode, 8 -> 16 -> 8 outputs per lane ahead of calls 2 and 5 of 8: the FIR
    histories, the oscillator and the demodulator state carry across kernels of either block."""
    C = 67
    n = (lead + 8) * N
    got, ref = run_family(name, C, N, n, switch_blocks({lead + 2: 16, lead + 5: 8}))
    assert_family_exact(name, got, ref, f"N={N} 8 -> 16 -> 8")
    check_audible(name, ref[0], n, N)
    if lead:
        assert np.abs(ref[0][:, lead * N:(lead + 1) * N]).max() > 0, "the switching stretch starts in silence"


def run_handoff(name, C, N, calls, mode, blocks=None, front_block=None):
    """run_pipelined without a synchronisation between calls -> asserts bit-exact, no give-up"""
    cfg, iq, r1, _, rdst = reference(name, C)
    n = calls * N
    if front_block is not None:
        blocks = dict(blocks or {})
        blocks[0] = front_block
    tmo = []
    a1, dst = run_pipelined(cfg, iq[:, :n], N, mode=mode, timeouts=tmo, blocks=blocks)
    assert_bitexact(a1, r1[:, :n], f"{name} mode {mode} N={N} blocks {blocks}")
    np.testing.assert_array_equal(dst, rdst[:, :n])
    assert tmo == [0]
    assert np.abs(r1[:, n - N:n]).max() > 0


SWITCH_HANDOFF = [("wide_p48_usb", 1), ("wide_p48_usb", 2), ("wide_p48_usb", 3), ("narrow_p35_lsb", 2)]


@pytest.mark.parametrize("name,mode", SWITCH_HANDOFF, ids=[f"{n}-mode{m}" for n, m in SWITCH_HANDOFF])
def test_front_block_switch_handoff(cuda, name, mode):
    """The block changed between calls of the event hand-off, the device hand-off and the persistent
    back end, inside and across the 4-call buffer groups, nothing synchronised by the caller: the
    arrival counters count front waves, whose number per group changes with the block."""
    run_handoff(name, 130, 256, 17, mode, blocks={3: 16, 6: 8, 9: 16, 13: 8})


# (mode, N, R): front waves that straddle two back-end groups (cpw 5: waves 12 and 25 of 26; cpw 10,
# 3, 1); the persistent back end takes calls of 8+ sub-calls (320 frames: 10, no multiple of its skew)
ODD_HANDOFF = [(2, 96, 8), (2, 96, 16), (2, 160, 8), (3, 320, 16), (3, 320, 8)]


@pytest.mark.parametrize("mode,N,R", ODD_HANDOFF, ids=[f"mode{m}-N{N}-R{R}" for m, N, R in ODD_HANDOFF])
def test_handoff_odd_call_sizes(cuda, mode, N, R):
    """Arrival counting with cpw that does not divide 64 (rx_front's add to both groups of a
    straddling wave, front_waves_of on the back end's side)."""
    run_handoff("wide_p48_usb", 130, N, 15, mode, front_block=R if R != 8 else None)


CHAIN_SIZES = [(name, N) for name in ("wide_p48_usb", "narrow_p35_lsb") for N in (96, 160, 192, 224)]


@pytest.mark.parametrize("name,N", CHAIN_SIZES, ids=[f"{n}-N={N}" for n, N in CHAIN_SIZES])
def test_chain_call_sizes(cuda, name, N):
    """rx_chain runs 64 / cpw front passes per wave and reads their LDS hand-off as lane == channel:
    a call size whose cpw does not divide 64 (96: 5, 160: 3) must be refused with UHSDR_UNSUPPORTED,
    the schedule unchanged, or else computed right; 192 (cpw 2, 32 passes, 16 idle lanes) must be
    accepted, so the run holds both outcomes."""
    import torch
    C, calls = 130, 8
    cfg, iq, r1, _, rdst = reference(name, C)
    n = calls * N
    chain = U.RxChain(cfg, channels=C, frames=N)
    before = chain.schedule
    try:
        chain.set_schedule(U.SCHEDULE_CHAIN)
        accepted = True
    except U.UhsdrError as e:
        accepted = False
        assert e.status == U.UHSDR_UNSUPPORTED
        assert chain.schedule == before
    print(f"{name} N={N}: CHAIN {'accepted' if accepted else 'refused (UHSDR_UNSUPPORTED)'}")
    if N == 192:
        assert accepted, "rx_chain must take 192-frame calls (two channels per wave, 32 passes)"
    if accepted:
        assert chain.schedule == U.SCHEDULE_CHAIN
        audio = torch.empty((C, N), dtype=torch.float32, device="cuda")
        dst = torch.empty((C, N, 2), dtype=torch.int32, device="cuda")
        a1 = np.empty((C, n), np.float32)
        d = np.empty((C, n, 2), np.int32)
        for k in range(calls):
            chain.process(torch.from_numpy(np.ascontiguousarray(iq[:, k * N:(k + 1) * N])).cuda(), audio, dst)
            torch.cuda.synchronize()
            a1[:, k * N:(k + 1) * N] = audio.cpu().numpy()
            d[:, k * N:(k + 1) * N] = dst.cpu().numpy()
        assert chain.schedule == U.SCHEDULE_CHAIN
        assert_bitexact(a1, r1[:, :n], f"{name} CHAIN N={N}")
        np.testing.assert_array_equal(d, rdst[:, :n])
        assert np.abs(r1[:, n - N:n]).max() > 0
    chain.close()


# (N, block asked for, calls): two lanes per channel; 1024 does not divide 1536; neither 8 nor 16.
# 32-frame calls run 8 calls (past the AGC ring), the refusal still between calls 1 and 2.
REFUSALS = [(32, 16, 8), (1536, 16, 4), (256, 12, 4)]


@pytest.mark.parametrize("N,R,calls", REFUSALS, ids=[f"N{N}-R{R}" for N, R, _ in REFUSALS])
def test_front_block_refusals_leave_handle_usable(cuda, N, R, calls):
    C, name = 67, "wide_p48_usb"
    refused = []

    def hook(chain, k):
        if k == 2:
            with pytest.raises(U.UhsdrError):
                chain.set_front_block(R)
            refused.append(k)

    n = calls * N
    got, ref = run_family(name, C, N, n, hook)
    assert refused == [2]
    assert_family_exact(name, got, ref, f"N={N} after set_front_block({R}) was refused")
    check_audible(name, ref[0], n, N)
