#!/usr/bin/env python3
"""Record tests/golden/psk_*.npz from the reference firmware's BPSK decoder.

Builds tools/psk/psk_driver.c against the reference objects and its psk.c (psk.mk, through
oracle/ref/Makefile) into a git-ignored or outside directory, generates the cases below with
uhsdr_amd.synth.psk_audio, runs each through the driver (one process per case: the demodulator's
statics never reset) and stores, per case:

  gen json                  psk_audio's arguments (the input is regenerated from them)
  message uint8 [k]         the bytes sent
  samples int32, crc32      length and crc32 of the float32 input
  speed_idx                 psk_ctrl_config
  chars uint8 [n]           the bytes UiDriver_TextMsgPutChar received
  char_sample int32 [n]     the index of the sample that emitted each
  expect, min_chars         what the recording shows, asserted here and by the loader
                            (tests/psk_cases.py): "sent" the message is in the printed bytes, "twice"
                            it is there twice, "garbled" it is not, "count" at least min_chars bytes
                            were printed, "nothing" none, "recorded" only the recording itself

and, for the decoder inside the receive chain (psk_chain_*.npz: tools/psk/psk_capture.c linked
with the reference harness and its main, run with mode=6 on a 12 ksps path), per case:

  gen json                  psk_iq's arguments (channel, frames, text, ...: the I/Q is regenerated)
  path, crc32               the filter path and the crc32 of the int32 I/Q frames
  tap_crc uint32 [calls]    crc32 of the 8 float32 samples each 32-frame call hands the demodulator
  tap_head float32 [256]    the first 256 of them raw
  chars, char_sample        as above, char_sample counting tap samples
  speed_idx; message        printed verbatim (asserted here)

  python3 tools/psk/make_psk_golden.py [--check] [--out DIR] [--ref /root/reference/mchf-eclipse]
"""
import json
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recording  # noqa: E402
from uhsdr_amd import synth  # noqa: E402

M31 = b"Hello de DL1ABC: 599, 73!"
M63 = b"CQ CQ de UHSDR, Pse k (QSL?) #7"
M125 = b"Test de DL1ABC: UR RST 599-579, QSL? Pwr 25W @ 14.070 MHz (73)! the quick brown fox"
SHORT = b"CQ de UHSDR k"


def case(name, message, speed_idx=2, expect="sent", min_chars=0, **gen):
    gen = dict(dict(baud=synth.PSK_SPEEDS[speed_idx]), **gen)
    return dict(name=name, message=bytes(message), speed_idx=speed_idx, expect=expect, min_chars=min_chars, gen=gen)


def cases():
    out = [
        case("clean31", M31, 0),
        case("clean63", M63, 1),
        case("clean125", M125, 2),
        case("chartable125", bytes(range(256)), 2),
        case("noisy_a", M125, 2, noise_sigma=500.0, seed=1, expect="count", min_chars=20),
        case("noisy_b", M125, 2, noise_sigma=800.0, seed=2, expect="garbled", min_chars=20),
        case("df0p5", M125, 2, df=0.5, expect="garbled"),
        case("df1", M125, 2, df=1.0, expect="garbled"),
        case("df2", M125, 2, df=2.0, expect="garbled"),
        case("tiny", M125, 2, amplitude=1e-26, expect="count", min_chars=30),
        case("floor", M125, 2, amplitude=1e-28, expect="nothing"),
        case("huge", M125, 2, amplitude=1e30),
        case("overflow", M125, 2, amplitude=1e34, expect="nothing"),
        case("idle60", M125, 2, idle_ones=60, expect="recorded"),
        case("burst", M63, 2, silence=60000, repeat=2, expect="twice"),
        case("silence", b"", 2, amplitude=0.0, lead=30000, expect="nothing"),
        case("midchar", M125, 2, offset=8 * 96 + 500, expect="recorded"),
    ]
    # the same text with the bit boundary at 8 offsets across one bit of 192 samples
    out += [case(f"offsets63_{k}", SHORT, 1, offset=24 * k) for k in range(8)]
    return out


def chain_cases():
    """P48 DIGI at BPSK31 and at BPSK125"""
    return [
        dict(name="chain_p48_31", path=48, speed_idx=0, channel=0, text="de UHSDR", nframes=96 * 2048),
        dict(name="chain_p48_125", path=48, speed_idx=2, channel=1, text="CQ CQ de UHSDR, 599 k", nframes=64 * 2048),
    ]


def chain_gen(c):
    return dict(channel=c["channel"], nframes=c["nframes"], text=c["text"], baud=synth.PSK_SPEEDS[c["speed_idx"]], lead=4800)


def chain_iq(gen):
    g = dict(gen)
    return np.ascontiguousarray(synth.psk_iq([g.pop("channel")], 0, g.pop("nframes"), g.pop("text"), **g)[0], dtype=np.int32)


def parse(res):
    res = res.split()
    return np.array(res[1::2], dtype=np.int64).astype(np.uint8), np.array(res[0::2], dtype=np.int32)


def record_chain(out, writer, tmp):
    rec = os.path.join(out, "psk_chain")
    for c in chain_cases():
        gen = chain_gen(c)
        iq = chain_iq(gen)
        fin, ftap, fchr = (os.path.join(tmp, c["name"] + x) for x in (".iq", ".tap", ".chr"))
        iq.tofile(fin)
        env = dict(os.environ, PSK_SPEED=str(c["speed_idx"]), PSK_TAP_LOG=ftap, PSK_CHAR_LOG=fchr)
        subprocess.run([rec, f"in={fin}", f"n={len(iq)}", "mode=6", f"path={c['path']}"], check=True, env=env)
        tap = np.fromfile(ftap, dtype=np.float32)
        assert len(tap) == len(iq) // 4, f"{c['name']}: {len(tap)} tap samples for {len(iq)} frames"
        chars, char_sample = parse(open(fchr).read())
        text = bytes(chars)
        print(f"{c['name']:18s} {len(iq):7d} frames   {text!r}")
        assert c["text"].encode() in text, f"{c['name']}: the reference did not print the message verbatim"
        tap_crc = np.array([zlib.crc32(tap[k:k + 8].tobytes()) for k in range(0, len(tap), 8)], dtype=np.uint32)
        writer.save(f"psk_{c['name']}.npz", gen=np.array(json.dumps(gen)), path=np.int32(c["path"]),
                    crc32=np.uint32(zlib.crc32(iq.tobytes())), tap_crc=tap_crc, tap_head=tap[:256].copy(),
                    speed_idx=np.int32(c["speed_idx"]), chars=chars, char_sample=char_sample, message=np.array(c["text"]))


def check_expectation(name, expect, min_chars, sent, printed):
    """what a recording must show to be worth keeping (tests/psk_cases.py asserts the same)"""
    if expect == "sent":
        assert sent in printed, f"{name}: the reference did not print the message"
    elif expect == "twice":
        assert printed.count(sent) == 2, f"{name}: the message is not there twice"
    elif expect == "garbled":
        assert sent not in printed, f"{name}: the reference printed the message"
    elif expect == "nothing":
        assert len(printed) == 0, f"{name}: the reference printed {printed!r}"
    assert len(printed) >= min_chars, f"{name}: only {len(printed)} bytes"


def main():
    a = recording.parse_args()
    out = recording.build(a, ["psk"], ["psk_driver", "psk_chain"])
    drv = os.path.join(out, "psk_driver")
    writer = recording.Recorder(a)

    with tempfile.TemporaryDirectory() as tmp:
        record_chain(out, writer, tmp)
        for c in cases():
            audio = synth.psk_audio(c["message"], **c["gen"])
            wav = os.path.join(tmp, c["name"] + ".f32")
            audio.tofile(wav)
            chars, char_sample = parse(subprocess.run([drv, wav, str(c["speed_idx"])], check=True, capture_output=True, text=True).stdout)
            printed = bytes(chars)
            print(f"{c['name']:14s} {len(audio):7d} samples {len(printed):4d} bytes  {printed[:100]!r}")
            check_expectation(c["name"], c["expect"], c["min_chars"], c["message"], printed)
            writer.save(f"psk_{c['name']}.npz", gen=np.array(json.dumps(c["gen"])),
                        message=np.frombuffer(c["message"], np.uint8), samples=np.int32(len(audio)),
                        crc32=np.uint32(zlib.crc32(audio.tobytes())), speed_idx=np.int32(c["speed_idx"]),
                        chars=chars, char_sample=char_sample, expect=np.array(c["expect"]), min_chars=np.int32(c["min_chars"]))
    writer.finish()


if __name__ == "__main__":
    main()
