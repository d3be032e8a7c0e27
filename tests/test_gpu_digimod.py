"""RTTY and BPSK modulators on the device (rttymod_gen / pskmod_gen) against the recordings of the
reference firmware (tests/golden/digimod_*.npz) and against the host handles, which
test_digimod_host.py holds to the same recordings.  Everything is int16-equal."""
import ctypes as C
import functools

import numpy as np
import pytest

from uhsdr_amd import digimod

from digimod_cases import check_outputs, check_samples, load_case, make, run_ops

pytestmark = pytest.mark.gpu

PAD = 0x5a5a
# fixtures of one parameter set whose text is put once, at the start; what follows a later op of
# theirs is not compared
GROUPS = {
    "rtty": ("rtty_s170_45_15", "rtty_altfigs", "rtty_lower_nocode", "rtty_idle", "rtty_eot"),
    "psk": ("psk_125_high", "psk_125_eot", "psk_125_idle"),
}
TOTAL = {"rtty": 90000, "psk": 150000}      # past the EOT of rtty_eot, past OFF of psk_125_eot
MOST = 130


def group(kind):
    return [load_case(n) for n in GROUPS[kind]]


def first_text(g):
    return g["ops"][0][1] if g["ops"][0][0] == "put" else b""


def texts(kind, channels):
    """The fixtures' texts and an empty queue in rotation; from the second round on the bytes of a
    text are rotated as well, so no two channels of a wave run alike."""
    base = [first_text(g) for g in group(kind)] + [b""]
    out = []
    for c in range(channels):
        t, r = base[c % len(base)], c // len(base)
        out.append(t[r % len(t):] + t[:r % len(t)] if t else t)
    return out


@functools.lru_cache(maxsize=None)
def host_ref(kind):
    """MOST channels on the host, once: samples [MOST][TOTAL], consumed, txoff_at, state"""
    mod = make(group(kind)[0], channels=MOST)
    mod.put_text(texts(kind, MOST))
    audio = mod.generate(TOTAL[kind])
    audio.setflags(write=False)
    ref = (audio, mod.consumed(), mod.txoff_at(), mod.state())
    mod.close()
    return ref


def generate(mod, total, sizes, torch):
    """`total` samples in calls of sizes[k % len(sizes)] into one tensor [C][total + 3]: an odd
    stride, so rows start at odd int16 offsets, and n < stride in every call"""
    audio = torch.full((mod.channels, total + 3), PAD, dtype=torch.int16, device="cuda")
    b = k = 0
    while b < total:
        m = min(sizes[k % len(sizes)], total - b)
        mod._call("process", C.c_void_p(audio.data_ptr() + 2 * b), m, total + 3)
        b, k = b + m, k + 1
    mod.synchronize()
    got = audio.cpu().numpy()
    assert (got[:, total:] == PAD).all()
    return got[:, :total]


def check_against_host(kind, mod, got):
    ref, consumed, txoff_at, state = host_ref(kind)
    ch, n = got.shape
    assert np.array_equal(got, ref[:ch, :n])
    if n == ref.shape[1]:
        assert np.array_equal(mod.consumed(), consumed[:ch])
        assert np.array_equal(mod.txoff_at(), txoff_at[:ch])
        assert np.array_equal(mod.state(), state[:ch])


@pytest.mark.parametrize("channels", [1, 63, 64, 65, MOST])
@pytest.mark.parametrize("kind", ["rtty", "psk"])
def test_channel_counts(cuda, kind, channels):
    import torch
    gs = group(kind)
    mod = make(gs[0], channels=channels, host=False)
    t = texts(kind, channels)
    assert mod.put_text(t).tolist() == [len(x) for x in t]
    got = generate(mod, TOTAL[kind], [2048], torch)
    check_against_host(kind, mod, got)
    for c, g in enumerate(gs[:channels]):
        first_gen = next(op[1] for op in g["ops"] if op[0] == "gen")
        check_samples(g, got[c], upto=min(first_gen, TOTAL[kind]))
    if kind == "psk" and channels > 1:
        assert mod.state()[1] == digimod.PSK_OFF and mod.txoff_at()[1] == load_case("psk_125_eot")["txoff_at"][0]
    mod.close()


@pytest.mark.parametrize("size,total", [(1, 3000), (32, 40000), (33, 40000), (257, None), (2048, None)])
@pytest.mark.parametrize("kind", ["rtty", "psk"])
def test_call_sizes(cuda, kind, size, total):
    import torch
    mod = make(group(kind)[0], channels=65, host=False)
    mod.put_text(texts(kind, 65))
    check_against_host(kind, mod, generate(mod, total or TOTAL[kind], [size], torch))
    mod.close()


@pytest.mark.parametrize("kind", ["rtty", "psk"])
def test_call_boundaries_inside_waits_and_windows(cuda, kind):
    """RTTY starts in the wait for the mark tone's zero crossing (the first start bit, from sample
    0, about 50 samples) and waits again at every change of bit; the BPSK preamble shapes every bit.
    Calls that end after 5, 25, 40 ... samples cut both, and so do the tile's 64 and its neighbours."""
    import torch
    mod = make(group(kind)[0], channels=64, host=False)
    mod.put_text(texts(kind, 64))
    check_against_host(kind, mod, generate(mod, 60000, [5, 20, 15, 1016, 10, 25, 333, 7, 1, 64, 65, 63, 128, 4097], torch))
    mod.close()


@pytest.mark.parametrize("name", ["rtty_late_cap8", "rtty_restart", "psk_63_dry", "psk_31_cap8", "psk_125_eot"])
def test_text_between_calls(cuda, name):
    """the fixture's ops (put between calls, StartTX / PrepareTx, a queue of 8) on the odd channels
    of 65, the even ones without text"""
    import torch
    g = load_case(name)
    mod = make(g, channels=65, host=False)
    new_audio = lambda stride: torch.full((65, stride), PAD, dtype=torch.int16, device="cuda")      # noqa: E731
    samples, accepted, after = run_ops(mod, g["ops"], chunk=8192, carries=lambda c: c % 2, new_audio=new_audio)
    idle = make(g)
    quiet, _, quiet_after = run_ops(idle, g["ops"], carries=lambda c: False)
    for c in (1, 33, 63):
        check_samples(g, samples[c])
        check_outputs(g, accepted, after, c)
    assert (samples[1::2] == samples[1]).all() and (samples[0::2] == quiet[0]).all()
    assert (accepted[:, 0::2] == 0).all()
    for got, want in zip(after, quiet_after):
        assert (got[:, 0::2] == want[:, :1]).all()
    idle.close()
    mod.close()


@pytest.mark.parametrize("kind", ["rtty", "psk"])
def test_reset_and_reuse(cuda, kind):
    import torch
    mod = make(group(kind)[0], channels=65, host=False)
    runs = []
    for _ in range(2):
        mod.put_text(texts(kind, 65))
        runs.append(generate(mod, 60000, [2048], torch))
        mod.reset()
        assert (mod.consumed() == 0).all() and (mod.txoff_at() == digimod.NO_TXOFF).all()
    assert np.array_equal(runs[0], runs[1])
    check_against_host(kind, mod, runs[0])
    mod.close()


@pytest.mark.parametrize("kind", ["rtty", "psk"])
def test_user_stream(cuda, kind):
    """Created on a stream of the caller's, moved to the default stream half way.  One new stream per
    modulator: a stream made here stays in the process, and the suite runs in one process."""
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.default_stream()
    mod = make(group(kind)[0], channels=65, host=False, stream=s1.cuda_stream)
    mod.put_text(texts(kind, 65))
    with torch.cuda.stream(s1):
        a = generate(mod, 30000, [2048], torch)
    mod.set_stream(s2.cuda_stream)
    with torch.cuda.stream(s2):
        b = generate(mod, 30000, [257], torch)
    check_against_host(kind, mod, np.concatenate([a, b], axis=1))
    mod.close()
