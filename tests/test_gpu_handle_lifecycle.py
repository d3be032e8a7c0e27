"""The life of a device handle of every per-channel module against its host twin: created on a
stream of its own, fed, reset, fed, moved to a second stream, fed, destroyed; every output equal
bit for bit after each feed.  65 channels are one full wave and one lane of the next, so the
partial last wave and every region of the one allocation are used; 1 channel is the smallest."""
import numpy as np
import pytest

from uhsdr_amd import cwdec, cwgen, digimod, nr, psk, rtty

pytestmark = pytest.mark.gpu

KINDS = ("cwdec", "rtty", "psk", "rttymod", "pskmod", "cwgen", "nr")


def rng():
    return np.random.default_rng(2024)


def dev(torch, a):
    """a on the device, complete: the upload runs on torch's stream, the kernels on the handle's"""
    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t


def feed_cwdec(torch, d, C):
    state = (rng().random((C, 3)) < 0.5).astype(np.uint8)
    d.process(state if d.host else dev(torch, state))
    return d.read()


def feed_f32(samples):
    def feed(torch, d, C):
        x = (rng().standard_normal((C, samples)) * 8000).astype(np.float32)
        d.process(x if d.host else dev(torch, x))
        out = d.read()
        return out + (d.symbol(),) if isinstance(d, psk.PskDecoder) else out
    return feed


def feed_mod(torch, m, C):
    m.put_text([b"RY%d" % (c % 10) for c in range(C)])
    m.start_tx() if isinstance(m, digimod.RttyModulator) else m.prepare_tx()
    audio = np.zeros((C, 64), np.int16)
    if m.host:
        m.process(audio)
    else:
        t = dev(torch, audio)
        m.process(t)
        m.synchronize()
        audio = t.cpu().numpy()
    return audio, m.consumed(), m.txoff_at(), m.state()


def feed_cwgen(torch, g, C):
    g.put_text([b"E%d" % (c % 10) for c in range(C)])
    keys = (rng().integers(0, 4, (C, 2))).astype(np.uint8)
    i, q = np.zeros((C, 64), np.float32), np.zeros((C, 64), np.float32)
    if g.host:
        g.process(keys, i, q)
    else:
        tk, ti, tq = dev(torch, keys), dev(torch, i), dev(torch, q)
        g.process(tk, ti, tq)
        g.synchronize()
        i, q = ti.cpu().numpy(), tq.cpu().numpy()
    return (i, q, g.flags(), g.consumed(), g.echo_total(), g.state()) + tuple(g.peek().values())


def feed_nr(torch, p, C):
    x = (rng().standard_normal((C, 2 * nr.FRAME)) * 3000).astype(np.float32)
    y = np.zeros_like(x)
    if p.host:
        p.process_frames(x, y)
    else:
        tx, ty = dev(torch, x), dev(torch, y)
        p.process_frames(tx, ty)
        p.synchronize()
        y = ty.cpu().numpy()
    return (y,) + p.state()


MAKE = {
    "cwdec": (lambda C, **kw: cwdec.CwDecoder(C, blocksize=8, text_capacity=8, **kw), feed_cwdec),
    "rtty": (lambda C, **kw: rtty.RttyDecoder(C, capacity=8, **kw), feed_f32(33)),
    "psk": (lambda C, **kw: psk.PskDecoder(C, speed=psk.SPEED_125, capacity=8, **kw), feed_f32(33)),
    "rttymod": (lambda C, **kw: digimod.RttyModulator(C, capacity=8, **kw), feed_mod),
    "pskmod": (lambda C, **kw: digimod.PskModulator(C, speed=psk.SPEED_125, capacity=8, **kw), feed_mod),
    "cwgen": (lambda C, **kw: cwgen.CwGenerator(C, speed=48, capacity=8, echo_capacity=8, **kw), feed_cwgen),
    "nr": (lambda C, **kw: nr.NrProcessor(C, **kw), feed_nr),
}


def same(got, want, what):
    assert len(got) == len(want)
    for k, (x, y) in enumerate(zip(got, want)):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        assert x.tobytes() == y.tobytes(), (what, k)


@pytest.mark.parametrize("C", [65, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_device_handle_follows_host_handle(cuda, kind, C):
    import torch
    make, feed = MAKE[kind]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d, h = make(C, stream=s1.cuda_stream), make(C, host=True)
    same(feed(torch, d, C), feed(torch, h, C), "fresh")
    d.reset()
    h.reset()
    same(feed(torch, d, C), feed(torch, h, C), "after reset")
    s1.synchronize()                    # the second stream's work comes after the first's
    d.set_stream(s2.cuda_stream)
    same(feed(torch, d, C), feed(torch, h, C), "on the second stream")
    d.close()
    h.close()
    assert d.handle is None and h.handle is None
