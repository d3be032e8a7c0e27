"""The CW generator on the device (cwgen_gen) against the recordings of the reference firmware
(tests/golden/cwgen_*.npz) and against the host handle, which test_cwgen_host.py holds to the same
recordings.  Everything is bit-equal.

Settings are handle-wide, so channels of one generator run fixtures of one setting: channel c runs
case c % K with its own keys and text.  A case without text or speed events starts (c // K) % 5 * 3
blocks late on its later channels, so that no two lanes of a wave are in step: a keyer that idles
after reset does nothing (all its timers are 0 and the tone's phase stands still), so the delayed
run is the recording moved by as many blocks."""
import functools

import numpy as np
import pytest

from uhsdr_amd import cwgen

from cwgen_cases import CASES, check_samples, load_case, make

pytestmark = pytest.mark.gpu

PAD = 7.0
B48 = ("tone_750", "text_paddle", "text_mid_element", "text_sentence")      # one setting: IAM_B, 48 wpm, rx_delay 0, queue of 32
WIDE = (B48, ("iam_a",), ("iam_b",), ("ultimate",), ("straight_repress",))
REST = tuple((n,) for n in CASES if n not in sum(WIDE, ()))


def plan(names, channels):
    """keys uint8 [C][B], the delay of every channel, and the events by block: {block: [(op, [channels])]}"""
    gs = [load_case(n) for n in names]
    K = len(gs)
    delay = [0 if gs[c % K]["events"] else (c // K) % 5 * 3 for c in range(channels)]
    B = -(-max(g["blocks"] + 12 for g in gs) // 64) * 64
    keys = np.zeros((channels, B), np.uint8)
    events = {}
    for c in range(channels):
        g = gs[c % K]
        keys[c, delay[c]:delay[c] + g["blocks"]] = g["keys"]
    for k, g in enumerate(gs):
        for b, op in g["events"]:
            events.setdefault(b, []).append((op, list(range(k, channels, K))))
    return gs, keys, delay, events


def run(gen, keys, events, sizes, torch):
    """the keys through `gen` in calls of sizes[k % len(sizes)] blocks, cut at every event as well.
    Device: into one tensor pair [C][32 B + 5], so rows start at odd offsets and n < stride."""
    C, B = keys.shape
    host = gen.host
    if host:
        i, q = np.full((C, 32 * B + 5), PAD, np.float32), np.full((C, 32 * B + 5), PAD, np.float32)
    else:
        i = torch.full((C, 32 * B + 5), PAD, dtype=torch.float32, device="cuda")
        q = torch.full((C, 32 * B + 5), PAD, dtype=torch.float32, device="cuda")
    flags = np.zeros((C, B), np.uint8)
    accepted = []
    b = k = 0
    while b < B:
        for op, chans in events.get(b, []):
            if op[0] == "put":
                accepted.append(gen.put_text([op[1] if c in chans else b"" for c in range(C)]))
            else:
                gen.set_speed(op[1], op[2])
        m = min([sizes[k % len(sizes)], B - b] + [e - b for e in events if e > b])
        kb = np.ascontiguousarray(keys[:, b:b + m])
        if host:
            gen._call("process_host", kb.ctypes.data, i[:, 32 * b:].ctypes.data, q[:, 32 * b:].ctypes.data, 32 * m, 32 * B + 5)
        else:
            kd = torch.from_numpy(kb).cuda()
            gen._call("process", kd.data_ptr(), i.data_ptr() + 128 * b, q.data_ptr() + 128 * b, 32 * m, 32 * B + 5)
        gen._blocks = m
        flags[:, b:b + m] = gen.flags()
        b, k = b + m, k + 1
    gen.synchronize()
    if not host:
        i, q = i.cpu().numpy(), q.cpu().numpy()
    assert (i[:, 32 * B:] == PAD).all() and (q[:, 32 * B:] == PAD).all()
    return dict(i=i[:, :32 * B], q=q[:, :32 * B], flags=flags, accepted=accepted, consumed=gen.consumed(), echo=gen.echo(),
                echo_total=gen.echo_total(), state=gen.state(), words=gen.peek())


def same(a, b):
    assert np.array_equal(a["i"].view(np.uint32), b["i"].view(np.uint32)) and np.array_equal(a["q"].view(np.uint32), b["q"].view(np.uint32))
    assert np.array_equal(a["flags"], b["flags"]) and np.array_equal(a["consumed"], b["consumed"]) and a["echo"] == b["echo"]
    assert np.array_equal(a["echo_total"], b["echo_total"]) and np.array_equal(a["state"], b["state"])
    assert all(np.array_equal(x, y) for x, y in zip(a["accepted"], b["accepted"])) and len(a["accepted"]) == len(b["accepted"])
    for k in cwgen.WORDS:
        assert np.array_equal(a["words"][k], b["words"][k]), k


def check_fixtures(names, channels, sizes, torch, host=False):
    gs, keys, delay, events = plan(names, channels)
    gen = make(gs[0], channels=channels, host=host)
    r = run(gen, keys, events, sizes, torch)
    gen.close()
    K = len(gs)
    for c in range(channels):
        g, d = gs[c % K], delay[c]
        n = g["blocks"]
        if c < K:
            check_samples(g, r["i"][c], r["q"][c])
            assert np.array_equal(r["flags"][c, :n], g["flags"]), g["name"]
            if K == 1:
                assert [int(a[c]) for a in r["accepted"]] == g["accepted"].tolist()
            # the run is longer than the recording: a word space may follow
            assert r["consumed"][c] == g["consumed"] and r["echo"][c].rstrip(b" ") == g["echo"].rstrip(b" "), (g["name"], r["echo"][c])
        else:
            for what in ("i", "q"):
                assert np.array_equal(r[what][c, 32 * d:32 * (d + n)].view(np.uint32), r[what][c % K, :32 * n].view(np.uint32)), (g["name"], c, what)
                assert not r[what][c, :32 * d].any()
            assert np.array_equal(r["flags"][c, d:d + n], g["flags"]) and r["consumed"][c] == g["consumed"]
            assert r["echo"][c].rstrip(b" ") == g["echo"].rstrip(b" ")
    return r


@pytest.mark.parametrize("channels,blocks", [(1, 64), (64, 8), (65, 64), (130, 64)])
@pytest.mark.parametrize("names", WIDE, ids=lambda n: n[0] if len(n) == 1 else "b48")
def test_fixtures_channel_counts(cuda, names, channels, blocks):
    """n = 2048 and n = 256 (64 and 8 blocks a call)"""
    import torch
    check_fixtures(names, channels, [blocks], torch)


@pytest.mark.parametrize("names", REST, ids=lambda n: n[0])
def test_fixtures_65_channels(cuda, names):
    import torch
    check_fixtures(names, 65, [64], torch)


@pytest.mark.parametrize("name", ["straight_long", "tone_1000", "straight_tap"])
def test_block_calls(cuda, name):
    """n = 32: one block a call"""
    import torch
    check_fixtures((name,), 65, [1], torch)


@functools.lru_cache(maxsize=None)
def b48_host():
    gs, keys, delay, events = plan(B48, 130)
    gen = make(gs[0], channels=130)
    r = run(gen, keys, events, [64], None)
    gen.close()
    for v in (r["i"], r["q"], r["flags"]):
        v.setflags(write=False)
    return r


@pytest.mark.parametrize("sizes", [[64], [8], [1, 8, 64, 3, 5, 2]], ids=["2048", "256", "mixed"])
def test_same_run_split_differently(cuda, sizes):
    """the four cases of one setting over 130 channels against the host handle's run, whatever the calls"""
    import torch
    gs, keys, delay, events = plan(B48, 130)
    gen = make(gs[0], channels=130, host=False)
    r = run(gen, keys, events, sizes, torch)
    gen.close()
    same(r, b48_host())


def random_keys(rng, channels, blocks):
    """piecewise constant lines: holds of 1 .. 40 blocks, half of them released"""
    keys = np.zeros((channels, blocks), np.uint8)
    for c in range(channels):
        b = 0
        while b < blocks:
            hold = int(rng.integers(1, 41))
            keys[c, b:b + hold] = rng.choice([0, 0, 0, 1, 2, 3])
            b += hold
    return keys


@pytest.mark.parametrize("mode", [cwgen.IAM_B, cwgen.IAM_A, cwgen.STRAIGHT, cwgen.ULTIMATE])
def test_random_keys_against_host(cuda, mode):
    """No recording exists for this one: the host handle, which has passed the recordings, is the
    reference.  130 channels x 4096 samples, every third channel with text and no keys until late."""
    import torch
    rng = np.random.default_rng(1234 + mode)
    C, B = 130, 128
    keys = random_keys(rng, C, B)
    keys[::3, :100] = 0
    text = [b"e it~5 " if c % 3 == 0 else b"" for c in range(C)]
    got = []
    for host in (True, False):
        gen = cwgen.CwGenerator(C, mode=mode, speed=48, weight=80, reverse=mode == cwgen.IAM_A, rx_delay=1, sidetone=620, capacity=8, echo_capacity=8, host=host)
        assert gen.put_text(text).tolist() == [len(t) for t in text]
        got.append(run(gen, keys, {}, [64] if host else [5, 64, 1, 30], torch))
        gen.close()
    same(got[1], got[0])
    assert got[0]["flags"].any() and (mode == cwgen.STRAIGHT or got[0]["echo_total"].any())


def test_reset_and_user_stream(cuda):
    """created on a stream of the caller's, moved to the default stream half way, reset and run again"""
    import torch
    gs, keys, delay, events = plan(("iam_b",), 65)
    keys = keys[:, :1024]
    s1, s2 = torch.cuda.Stream(), torch.cuda.default_stream()
    gen = make(gs[0], channels=65, host=False, stream=s1.cuda_stream)
    with torch.cuda.stream(s1):
        a = run(gen, keys[:, :512], {}, [64], torch)
    gen.set_stream(s2.cuda_stream)
    with torch.cuda.stream(s2):
        b = run(gen, keys[:, 512:], {}, [8], torch)
        gen.reset()
        assert not gen.consumed().any() and not gen.echo_total().any() and all(not v.any() for v in gen.peek().values())
        again = run(gen, keys, {}, [64], torch)
    gen.close()
    for what in ("i", "q", "flags"):
        assert np.array_equal(np.concatenate([a[what], b[what]], axis=1), again[what])
    check_samples(gs[0], again["i"][0], again["q"][0], blocks=1024)


def test_process_wrapper_on_the_device(cuda):
    """CwGenerator.process itself with torch tensors and n < stride, and its shape and dtype checks"""
    import torch
    g = load_case("straight_long")
    B = 64
    keys = np.zeros((3, B), np.uint8)
    keys[1] = g["keys"][:B]
    gen = make(g, channels=3, host=False)
    i = torch.full((3, 32 * B + 7), PAD, dtype=torch.float32, device="cuda")
    q = torch.full((3, 32 * B + 7), PAD, dtype=torch.float32, device="cuda")
    gen.process(torch.from_numpy(keys).cuda(), i, q, 32 * B)
    gen.synchronize()
    hi, hq = i.cpu().numpy(), q.cpu().numpy()
    assert (hi[:, 32 * B:] == PAD).all() and (hq[:, 32 * B:] == PAD).all() and not hi[0, :32 * B].any() and not hq[2, :32 * B].any()
    check_samples(g, hi[1], hq[1], blocks=B)
    assert np.array_equal(gen.flags()[1], g["flags"][:B])
    with pytest.raises(ValueError):
        gen.process(torch.from_numpy(keys[:, :5]).cuda(), i, q, 32 * B)
    with pytest.raises(ValueError):
        gen.process(torch.from_numpy(keys).cuda(), i.double(), q, 32 * B)
    with pytest.raises(ValueError):
        gen.process(torch.from_numpy(keys).cuda(), i[:2], q[:2], 32 * B)
    gen.close()
