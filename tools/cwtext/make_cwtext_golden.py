#!/usr/bin/env python3
"""Record tests/golden/cwtext_*.npz from the reference firmware's CW decoder.

Builds tools/cwtext/cwtext_driver.c against the reference objects (cwtext.mk, through
oracle/ref/Makefile) into a git-ignored or outside directory, keys the cases below as 12 ksps
audio, runs each through the driver and stores, per case:

  state uint8 [blocks]      ads.CW_signal after each completed block (the decoder's input)
  blocksize, spikecancel    cw_decoder_config
  chars uint8 [n]           the bytes UiDriver_TextMsgPutChar received
  char_block int32 [n]      the block during which each arrived
  speed uint8 [blocks]      cw_decoder_config.speed after each block
  message                   what was keyed

and cwtext_chartable.npz: CwGen_CharacterIdFunc for every code of 0 to 9 elements.

  python3 tools/cwtext/make_cwtext_golden.py [--check] [--out DIR] [--ref /root/reference/mchf-eclipse]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recording  # noqa: E402
from uhsdr_amd.synth import morse_keying  # noqa: E402

RATE = 12000.0
TONE, AMPLITUDE, THRESH = 750.0, 100.0, 1000

M1 = "CQ CQ DE UHSDR"
M2 = "PARIS QUIZ 73 K"
M3 = "HI TAJ IRAQ YOU REV QUIZ 599 <AR> TEST <HH> <SK> 1234567890 <KN> "


def runs_of(text, wpm, jitter=0.0, rng=None):
    """(key down?, seconds) runs of a message; every run's length jittered by +-jitter."""
    unit = 1.2 / wpm
    out = []
    for down, u in morse_keying(text):
        k = 1.0 + (jitter * (2.0 * rng.random() - 1.0) if jitter else 0.0)
        out.append((down, u * unit * k))
    return out


def audio_of(runs, lead=1.0, tail=4.5):
    """12 ksps float32 audio: the tone, phase continuous, keyed hard by the runs."""
    runs = [(False, lead)] + list(runs) + [(False, tail)]
    edges = np.rint(np.cumsum([0.0] + [s * RATE for _, s in runs])).astype(np.int64)
    key = np.zeros(int(edges[-1]), dtype=np.float64)
    for (down, _), a, b in zip(runs, edges[:-1], edges[1:]):
        if down:
            key[a:b] = 1.0
    return key


def tone(key):
    n = np.arange(len(key), dtype=np.float64)
    return (AMPLITUDE * key * np.sin(2.0 * np.pi * TONE / RATE * n)).astype(np.float32)


def inject(key, blocksize, rng, every=1.7):
    """one-block spikes in spaces and one-block dropouts in marks, about every `every` seconds"""
    key = key.copy()
    pos = int(1.2 * RATE)
    while pos + blocksize < len(key):
        key[pos:pos + blocksize] = 1.0 - round(float(key[pos:pos + blocksize].mean()))
        pos += int(every * RATE * (0.6 + 0.8 * rng.random()))
    return key


def cases():
    out = []
    clean = [(12, 88, M1), (20, 60, M2), (30, 128, M1), (35, 88, M2), (20, 128, M2), (30, 60, M1),
             (12, 60, M2), (35, 128, M1), (20, 88, M1)]
    for wpm, bs, msg in clean:
        out.append(dict(name=f"clean{wpm}_b{bs}", blocksize=bs, spikecancel=0, noisecancel=1, message=msg, reps=6,
                        key=audio_of(runs_of((msg + " ") * 6, wpm)), clean=True))
    out.append(dict(name="mixed20_b88", blocksize=88, spikecancel=0, noisecancel=1, message=M3, reps=4,
                    key=audio_of(runs_of(M3 * 4, 20))))
    rng = np.random.default_rng(1973)
    out.append(dict(name="hand18_b88", blocksize=88, spikecancel=0, noisecancel=1, message=M1 + " PSE K", reps=6,
                    key=audio_of(runs_of((M1 + " PSE K ") * 6, 18, 0.30, rng))))
    for sc, bs in ((0, 88), (1, 60), (2, 88)):
        rng = np.random.default_rng(100 + sc)
        key = inject(audio_of(runs_of((M2 + " ") * 6, 20)), bs, rng)
        out.append(dict(name=f"spikes{sc}_b{bs}", blocksize=bs, spikecancel=sc, noisecancel=0, message=M2, reps=6, key=key))
    # 5 s of silence after a character ending in a dot (S) and after one ending in a dash (K)
    r = (runs_of((M1 + " ") * 3 + "PARIS", 20)[:-1] + [(False, 5.0)] + runs_of((M1 + " ") * 2 + "PARIS QUIZ 73 K", 20)[:-1]
         + [(False, 5.0)] + runs_of((M1 + " ") * 2, 20))
    out.append(dict(name="silence20_b88", blocksize=88, spikecancel=0, noisecancel=1, message=M1, reps=7, key=audio_of(r)))
    r = runs_of((M1 + " ") * 3, 20) + [(True, 3.0), (False, 0.42)] + runs_of((M1 + " ") * 3, 20)
    out.append(dict(name="stuck20_b88", blocksize=88, spikecancel=0, noisecancel=1, message=M1, reps=6, key=audio_of(r)))
    r = runs_of((M1 + " ") * 4, 15) + runs_of((M1 + " ") * 5, 30)
    out.append(dict(name="speed15to30_b88", blocksize=88, spikecancel=0, noisecancel=1, message=M1, reps=9, key=audio_of(r)))
    return out


def main():
    a = recording.parse_args()
    out = recording.build(a, ["cwtext"], ["cwtext"])
    drv = os.path.join(out, "cwtext_driver")
    writer = recording.Recorder(a)

    rows = [l.split() for l in subprocess.run([drv, "table"], check=True, capture_output=True, text=True).stdout.splitlines()]
    writer.save("cwtext_chartable.npz", code=np.array([int(r[0]) for r in rows], dtype=np.uint32),
                char=np.array([int(r[1]) for r in rows], dtype=np.uint8))

    any_hash = any_corrected = False
    with tempfile.TemporaryDirectory() as tmp:
        for c in cases():
            wav = os.path.join(tmp, c["name"] + ".f32")
            tone(c["key"]).tofile(wav)
            res = subprocess.run([drv, "run", wav, str(c["blocksize"]), str(THRESH), str(c["noisecancel"]), str(c["spikecancel"]),
                                  str(int(TONE))], check=True, capture_output=True, text=True).stdout.splitlines()
            state, speed, chars, char_block = [], [], [], []
            for b, line in enumerate(res):
                f = [int(x) for x in line.split()]
                state.append(f[0]); speed.append(f[1])
                for ch in f[2:]:
                    chars.append(ch); char_block.append(b)
            text = bytes(chars).decode("latin-1")
            print(f"{c['name']:18s} {len(state):6d} blocks  {text!r}")
            any_hash |= "#" in text
            if c.get("clean"):
                want = " ".join([c["message"]] * (c["reps"] - 2))
                # (the very last character stays pending when the ring slot the time-out reads, :672, holds a mark)
                assert text.rstrip().endswith((want, want[:-1])), \
                    f"{c['name']}: the keyed message is not reproduced from its third repetition on"
            elif c["name"].startswith(("hand", "spikes", "stuck", "speed", "silence", "mixed")):
                spelled = c["message"].replace("<AR>", "ar").replace("<SK>", "sk").replace("<KN>", "kn").replace("<HH>", "err")
                any_corrected |= text.count(spelled.strip()) < c["reps"]
            writer.save(f"cwtext_{c['name']}.npz", state=np.array(state, dtype=np.uint8),
                        blocksize=np.int32(c["blocksize"]), spikecancel=np.int32(c["spikecancel"]),
                        chars=np.array(chars, dtype=np.uint8), char_block=np.array(char_block, dtype=np.int32),
                        speed=np.array(speed, dtype=np.uint8), message=np.array(c["message"]),
                        noisecancel=np.int32(c["noisecancel"]), thresh=np.int32(THRESH))
    assert any_hash, "no case emits '#'"
    assert any_corrected, "no case emits text that differs from what was keyed"
    writer.finish()


if __name__ == "__main__":
    main()
