"""The host side every per-channel module shares, pinned through the C ABI on host handles: what
each entry point refuses, with which status and which text of uhsdr_last_error(), that a null
handle's synchronize and destroy leave the error text alone, and that reset gives back a fresh
handle.  The seven kinds: cwdec, rtty, psk, rttymod, pskmod, cwgen, nr.  The texts are literals:
this file holds on any library with the same ABI, before and after the host code moves."""
import ctypes as C

import numpy as np
import pytest

import uhsdr_amd as U
from uhsdr_amd import _abi, cwdec, cwgen, digimod, nr, psk, rtty, synth

ARG, LEN = _abi.UHSDR_ARGUMENT_ERROR, _abi.UHSDR_LENGTH_ERROR
KINDS = ("cwdec", "rtty", "psk", "rttymod", "pskmod", "cwgen", "nr")


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def cw_cfg(**kw):
    d = dict(keyer_mode=0, keyer_speed=20, keyer_weight=100, paddle_reverse=0, rx_delay=8, sidetone_freq=750)
    d.update(kw)
    return cwgen._Config(*[d[k] for k, _ in cwgen._Config._fields_])


# per kind: the create_host arguments that work (without the handle), as a dict in call order, and
# the refused variants of them: (overrides, text)
CREATE = {
    "cwdec": (dict(channels=4, blocksize=88, spikecancel=0, capacity=64), [
        (dict(channels=0), "cwdec: bad argument"),
        (dict(capacity=7), "cwdec: text_capacity 7 below 8"),
        (dict(blocksize=7), "cwdec: blocksize 7 not 8 .. 128"),
        (dict(blocksize=129), "cwdec: blocksize 129 not 8 .. 128"),
        (dict(spikecancel=3), "cwdec: spikecancel 3 not 0 .. 2"),
        (dict(spikecancel=-1), "cwdec: spikecancel -1 not 0 .. 2")]),
    "rtty": (dict(channels=4, shift=1, speed=0, stopbits=1, atc=0, capacity=64), [
        (dict(channels=0), "rtty: bad argument"),
        (dict(capacity=7), "rtty: text_capacity 7 below 8"),
        (dict(shift=6), "rtty: shift_idx 6 not 0 .. 5"),
        (dict(shift=-1), "rtty: shift_idx -1 not 0 .. 5"),
        (dict(speed=2), "rtty: speed_idx 2 not 0 .. 1"),
        (dict(stopbits=3), "rtty: stopbits_idx 3 not 0 .. 2")]),
    "psk": (dict(channels=4, speed=0, capacity=64), [
        (dict(channels=0), "psk: bad argument"),
        (dict(capacity=7), "psk: text_capacity 7 below 8"),
        (dict(speed=3), "psk: speed_idx 3 not 0 .. 2"),
        (dict(speed=-1), "psk: speed_idx -1 not 0 .. 2")]),
    "rttymod": (dict(channels=4, shift=1, speed=0, stopbits=1, capacity=64), [
        (dict(channels=0), "rttymod: bad argument"),
        (dict(capacity=7), "rttymod: text_capacity 7 below 8"),
        (dict(shift=6), "rttymod: shift_idx 6, speed_idx 0, stopbits_idx 1 not 0 .. 5, 0 .. 1, 0 .. 2"),
        (dict(speed=2), "rttymod: shift_idx 1, speed_idx 2, stopbits_idx 1 not 0 .. 5, 0 .. 1, 0 .. 2"),
        (dict(stopbits=3), "rttymod: shift_idx 1, speed_idx 0, stopbits_idx 3 not 0 .. 5, 0 .. 1, 0 .. 2")]),
    "pskmod": (dict(channels=4, speed=0, capacity=64), [
        (dict(channels=0), "pskmod: bad argument"),
        (dict(capacity=7), "pskmod: text_capacity 7 below 8"),
        (dict(speed=3), "pskmod: speed_idx 3 not 0 .. 2")]),
    "cwgen": (dict(channels=4, cfg={}, capacity=16, echo_capacity=16), [
        (dict(channels=0), "cwgen: bad argument"),
        (dict(cfg=None), "cwgen: bad argument"),
        (dict(capacity=7), "cwgen: text_capacity 7 or echo_capacity 16 below 8"),
        (dict(echo_capacity=7), "cwgen: text_capacity 16 or echo_capacity 7 below 8"),
        (dict(cfg=dict(keyer_mode=4)), "cwgen: keyer_mode 4, rx_delay 8, sidetone_freq 750 not 0 .. 3, 0 .. 50, 400 .. 1000"),
        (dict(cfg=dict(rx_delay=51)), "cwgen: keyer_mode 0, rx_delay 51, sidetone_freq 750 not 0 .. 3, 0 .. 50, 400 .. 1000"),
        (dict(cfg=dict(sidetone_freq=399)), "cwgen: keyer_mode 0, rx_delay 8, sidetone_freq 399 not 0 .. 3, 0 .. 50, 400 .. 1000"),
        (dict(cfg=dict(keyer_speed=4)), "cwgen: keyer_speed 4, keyer_weight 100 not 5 .. 48, 50 .. 150"),
        (dict(cfg=dict(keyer_weight=151)), "cwgen: keyer_speed 20, keyer_weight 151 not 5 .. 48, 50 .. 150")]),
    "nr": (dict(channels=4, cfg={}), [
        (dict(channels=0), "nr: bad argument"),
        (dict(cfg=None), "nr: bad argument"),
        (dict(cfg=dict(alpha=1.5)), "nr: alpha 1.5 outside 0..1"),
        (dict(cfg=dict(asnr=1)), "nr: asnr 1 outside 2..30"),
        (dict(cfg=dict(width=6)), "nr: width 6 outside 1..5"),
        (dict(cfg=dict(power_threshold_int=9)), "nr: power_threshold_int 9 outside 10..100"),
        (dict(cfg=dict(sample_rate=8000)), "nr: sample_rate 8000: 6000 or 12000"),
        (dict(cfg=dict(width_hz=-1)), "nr: filter width -1 / offset 1650 out of range"),
        (dict(cfg=dict(offset_hz=65536)), "nr: filter width 2700 / offset 65536 out of range")]),
}


def create_args(kind, **over):
    """the create_host arguments of a kind as ctypes values, and what keeps them alive"""
    d = dict(CREATE[kind][0])
    d.update(over)
    if "cfg" in d and d["cfg"] is not None:
        cfg = cw_cfg(**d["cfg"]) if kind == "cwgen" else nr.nr_config(**d["cfg"])
        d["cfg"] = C.byref(cfg)
    return list(d.values())


def create(lib, kind, out, **over):
    return getattr(lib, f"uhsdr_{kind}_create_host")(*create_args(kind, **over), out)


def err(lib):
    return lib.uhsdr_last_error().decode()


def refused(lib, status, want, text):
    assert status == want
    assert err(lib) == text


# per kind: how the row calls look.  `who` heads the texts of the run checks; `proc` / `proc_host`
# are the device and host entries; rows(C, stride) makes their pointer arguments; over / under are
# (n, text) for n > stride and n < 0 on a row of 16 (64 for cwgen); `use` ends the refusal of the
# device entry on a host handle; `stream_who` heads set_stream's.
def f32(channels, stride):
    return [np.zeros((channels, stride), np.float32)]


RUN = {
    "cwdec": dict(rows=lambda c, s: [np.zeros((c, s), np.uint8)], stride=16,
                  over=(17, "cwdec: 17 blocks do not fit a row of 16"), under=(-1, "cwdec: -1 blocks do not fit a row of 16"),
                  kind="cwdec: host handle, use uhsdr_cwdec_process_host", stream="cwdec: not a device handle"),
    "rtty": dict(rows=f32, stride=16,
                 over=(17, "rtty: 17 samples do not fit a row of 16"), under=(-1, "rtty: -1 samples do not fit a row of 16"),
                 kind="rtty: host handle, use uhsdr_rtty_process_host", stream="rtty: not a device handle"),
    "psk": dict(rows=f32, stride=16,
                over=(17, "psk: 17 samples do not fit a row of 16"), under=(-1, "psk: -1 samples do not fit a row of 16"),
                kind="psk: host handle, use uhsdr_psk_process_host", stream="psk: not a device handle"),
    "rttymod": dict(rows=lambda c, s: [np.zeros((c, s), np.int16)], stride=16,
                    over=(17, "digimod: 17 samples do not fit a row of 16"), under=(-1, "digimod: -1 samples do not fit a row of 16"),
                    kind="digimod: host handle, use the _process_host call", stream="digimod: not a device handle"),
    "pskmod": dict(rows=lambda c, s: [np.zeros((c, s), np.int16)], stride=16,
                   over=(17, "digimod: 17 samples do not fit a row of 16"), under=(-1, "digimod: -1 samples do not fit a row of 16"),
                   kind="digimod: host handle, use the _process_host call", stream="digimod: not a device handle"),
    "cwgen": dict(rows=lambda c, s: [np.zeros((c, s // 32), np.uint8), np.zeros((c, s), np.float32), np.zeros((c, s), np.float32)], stride=64,
                  over=(96, "cwgen: 96 samples do not fit a row of 64"), under=(-32, "cwgen: -32 samples do not fit a row of 64"),
                  kind="cwgen: host handle, use the _process_host call", stream="digimod: not a device handle"),
    "nr": dict(rows=lambda c, s: f32(c, s) + f32(c, s), stride=16,
               over=(24, "nr: 24 samples: a multiple of 8 that fits a row of 16"), under=(-8, "nr: -8 samples: a multiple of 8 that fits a row of 16"),
               kind="nr: host handle, use uhsdr_nr_process_host", stream="nr: not a device handle"),
}


@pytest.mark.parametrize("kind", KINDS)
def test_create_refusals(kind):
    lib = U.load()
    h = C.c_void_p()
    for over, text in CREATE[kind][1]:
        refused(lib, create(lib, kind, C.byref(h), **over), ARG, text)
        # the device entry refuses the same before any device call
        args = create_args(kind, **over)
        refused(lib, getattr(lib, f"uhsdr_{kind}_create")(*args, None, C.byref(h)), ARG, text)
    refused(lib, create(lib, kind, None), ARG, f"{kind}: bad argument")
    assert create(lib, kind, C.byref(h)) == 0
    assert getattr(lib, f"uhsdr_{kind}_destroy")(h) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_run_refusals(kind):
    lib = U.load()
    f = lambda name: getattr(lib, f"uhsdr_{kind}_{name}")     # noqa: E731
    r = RUN[kind]
    h = C.c_void_p()
    assert create(lib, kind, C.byref(h)) == 0
    arrays = r["rows"](4, r["stride"])
    rows = [ptr(a) for a in arrays]
    ok = r["stride"]
    for k in range(len(rows)):          # each row pointer null in turn
        refused(lib, f("process_host")(h, *[None if j == k else p for j, p in enumerate(rows)], ok, ok), ARG, "null argument")
    refused(lib, f("process_host")(h, *rows, r["over"][0], ok), LEN, r["over"][1])
    refused(lib, f("process_host")(h, *rows, r["under"][0], ok), LEN, r["under"][1])
    refused(lib, f("process")(h, *rows, ok, ok), ARG, r["kind"])
    refused(lib, f("set_stream")(h, None), ARG, r["stream"])
    assert f("process_host")(h, *rows, 0, ok) == 0
    assert f("process_host")(h, *rows, ok, ok) == 0
    assert f("synchronize")(h) == 0
    assert f("destroy")(h) == 0
    # a null handle
    refused(lib, f("process_host")(None, *rows, ok, ok), ARG, "null argument")
    refused(lib, f("reset")(None), ARG, "null handle")
    outputs = {"cwdec": 3, "rtty": 2, "psk": 3, "rttymod": 3, "pskmod": 3, "cwgen": 5}
    if kind == "nr":
        refused(lib, lib.uhsdr_nr_state(None, None, None, None), ARG, "null handle")
    else:
        refused(lib, f("outputs")(None, *[None] * outputs[kind]), ARG, "null handle")
    refused(lib, f("set_stream")(None, None), ARG, r["stream"])
    # synchronize and destroy of a null handle set no text
    refused(lib, f("reset")(None), ARG, "null handle")
    marker = err(lib)
    assert f("synchronize")(None) == ARG and err(lib) == marker
    assert f("destroy")(None) == ARG and err(lib) == marker
    refused(lib, create(lib, kind, C.byref(h), channels=0), ARG, f"{kind}: bad argument")
    assert f("synchronize")(None) == ARG and f("destroy")(None) == ARG and err(lib) == f"{kind}: bad argument"


def test_nr_frames_refusals():
    """the noise reduction's second pair of row entries"""
    lib = U.load()
    h = C.c_void_p()
    assert create(lib, "nr", C.byref(h)) == 0
    x, y = np.zeros((4, 128), np.float32), np.zeros((4, 128), np.float32)
    refused(lib, lib.uhsdr_nr_process_frames_host(h, None, ptr(y), 1, 128), ARG, "null argument")
    refused(lib, lib.uhsdr_nr_process_frames_host(h, ptr(x), None, 1, 128), ARG, "null argument")
    refused(lib, lib.uhsdr_nr_process_frames_host(h, ptr(x), ptr(y), 2, 128), LEN, "nr: 2 frames of 128 samples do not fit a row of 128")
    refused(lib, lib.uhsdr_nr_process_frames_host(h, ptr(x), ptr(y), -1, 128), LEN, "nr: -1 frames of 128 samples do not fit a row of 128")
    refused(lib, lib.uhsdr_nr_process_frames(h, ptr(x), ptr(y), 1, 128), ARG, "nr: host handle, use uhsdr_nr_process_frames_host")
    refused(lib, lib.uhsdr_nr_process_frames_host(None, ptr(x), ptr(y), 1, 128), ARG, "null argument")
    assert lib.uhsdr_nr_process_frames_host(h, ptr(x), ptr(y), 1, 128) == 0
    assert lib.uhsdr_nr_destroy(h) == 0


# ---- a reset handle is a fresh handle ----

CH = 5


def noise(n, scale, seed=11):
    return np.ascontiguousarray(np.random.default_rng(seed).standard_normal((CH, n)).astype(np.float32) * np.float32(scale))


def keyed(blocks):
    """a 20 wpm message, one byte per 88-sample block at 12 ksps, starting later channel by channel"""
    pat = synth.morse_envelope("CQ DE TEST", 20.0, 12000.0 / 88)
    row = np.tile(pat, blocks // len(pat) + 2)
    return np.ascontiguousarray(np.stack([np.concatenate([np.zeros(3 * c + 3, np.uint8), row])[:blocks] for c in range(CH)]))


def run_cwdec(d):
    d.process(keyed(3000))
    return d.read()


def run_rtty(d):
    d.process(noise(3000, 8000.0))
    return d.read()


def run_psk(d):
    d.process(noise(1999, 8000.0))        # no whole number of symbols: a clock that is not rewound shows
    return d.read() + (d.symbol(),)


def run_mod(m):
    m.put_text([b"RYRY de %d" % c for c in range(CH)])
    if isinstance(m, digimod.RttyModulator):
        m.start_tx()
    else:
        m.prepare_tx()
    return m.generate(4001), m.consumed(), m.txoff_at(), m.state()


def run_cwgen(g):
    g.put_text([b"E T%d" % c for c in range(CH)])
    keys = np.zeros((CH, 300), np.uint8)
    keys[1, 100:140] = cwgen.DIT
    i, q = g.generate(keys)
    return (i, q, g.flags(), g.consumed(), g.echo_total(), g.state()) + tuple(g.peek().values()) + tuple(np.frombuffer(e, np.uint8) for e in g.echo())


def run_nr(p):
    x = noise(7 * nr.FRAME, 3000.0)
    y = np.zeros_like(x)
    p.process_frames(x, y)
    z = np.zeros((CH, 800), np.float32)
    p.process(np.ascontiguousarray(x[:, :800]), z)
    return (y, z) + p.state()


ROUND = {
    "cwdec": (lambda: cwdec.CwDecoder(CH, blocksize=88, host=True), run_cwdec),
    "rtty": (lambda: rtty.RttyDecoder(CH, host=True), run_rtty),
    "psk": (lambda: psk.PskDecoder(CH, speed=psk.SPEED_125, host=True), run_psk),
    "rttymod": (lambda: digimod.RttyModulator(CH, host=True), run_mod),
    "pskmod": (lambda: digimod.PskModulator(CH, speed=psk.SPEED_125, host=True), run_mod),
    "cwgen": (lambda: cwgen.CwGenerator(CH, speed=30, host=True), run_cwgen),
    "nr": (lambda: nr.NrProcessor(CH, host=True), run_nr),
}


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_reset_gives_a_fresh_handle(kind):
    make, run = ROUND[kind]
    a = make()
    first = run(a)
    assert any(x.any() for x in first)
    a.reset()
    if kind == "nr":
        ft, nn, pr = a.state()
        assert (ft == 1).all() and (nn == 0).all() and (pr == 0).all()
    second = run(a)
    same(first, second)
    b = make()
    same(run(b), second)
    if kind in ("cwdec", "rtty", "psk"):
        assert (a.outputs.seen == 0).all()
    a.close()
    b.close()


def test_round_trips_are_not_trivial():
    """what the equalities above compare has content: text came out, symbols were decided, the
    stream state of psk moved"""
    d = ROUND["cwdec"][0]()
    text, total, wpm = run_cwdec(d)
    assert total.min() > 0
    d.close()
    p = ROUND["psk"][0]()
    once = run_psk(p)
    again = run_psk(p)          # no reset: the clock is mid-symbol, the same input decides elsewhere
    assert once[2].any() and once[2].tobytes() != again[2].tobytes()
    p.close()
    g = ROUND["cwgen"][0]()
    out = run_cwgen(g)
    assert out[3].min() > 0 and out[4].min() > 0
    g.close()
