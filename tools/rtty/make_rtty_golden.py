#!/usr/bin/env python3
"""Record tests/golden/rtty_*.npz from the reference firmware's RTTY decoder.

Builds tools/rtty/rtty_driver.c against the reference objects (rtty.mk, through
oracle/ref/Makefile) into a git-ignored or outside directory, generates the cases below with
uhsdr_amd.synth.rtty_audio, runs each through the driver (one process per case: the demodulator's
statics never reset) and stores, per case:

  gen json                  rtty_audio's arguments (the input is regenerated from them)
  bits_level, bits_length   the line's runs where the case is not plain text
  samples int32, crc32      length and crc32 of the float32 input
  shift_idx, speed_idx, stopbits_idx, atc_disable     rtty_ctrl_config
  chars uint8 [n]           the bytes UiDriver_TextMsgPutChar received
  char_sample int32 [n]     the index of the sample that emitted each
  message                   what was sent; verbatim != 0: the reference printed it verbatim

and, for the decoder inside the receive chain (rtty_chain_*.npz: tools/rtty/rtty_capture.c linked
with the reference harness and its main, run with mode=6 on a 12 ksps path), per case:

  gen json                  rtty_iq's arguments (channel, frames, text, ...: the I/Q is regenerated)
  path, crc32               the filter path and the crc32 of the int32 I/Q frames
  tap_crc uint32 [calls]    crc32 of the 8 float32 samples each 32-frame call hands the demodulator
  tap_head float32 [256]    the first 256 of them raw
  chars, char_sample        as above, char_sample counting tap samples
  shift_idx, ...            rtty_ctrl_config; message: printed verbatim (asserted here)

  python3 tools/rtty/make_rtty_golden.py [--check] [--out DIR] [--ref /root/reference/mchf-eclipse]
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

M1 = "RYRYRY CQ CQ DE UHSDR UHSDR K"
M2 = "THE QUICK BROWN FOX 0123456789"
M3 = "DE DL1ABC: UR RST 599-599 (73)\r\nQSL? $4.50 #7 & 'OK' /AR;\r\nBELL\a END."


def case(name, message, shift_idx=1, speed_idx=0, stopbits_idx=1, atc_disable=0, verbatim=True, bits=None, **gen):
    gen = dict(dict(shift=synth.RTTY_SHIFTS[shift_idx], baud=synth.RTTY_SPEEDS[speed_idx],
                    stopbits=synth.RTTY_STOPBITS[stopbits_idx]), **gen)
    return dict(name=name, message=message, shift_idx=shift_idx, speed_idx=speed_idx, stopbits_idx=stopbits_idx,
                atc_disable=atc_disable, verbatim=verbatim, bits=bits, gen=gen)


def broken_stop_bits():
    """M1, then a character whose stop bit is a space (a break of three bit times), then M2"""
    l1, n1 = synth.baudot_bits(M1 + " E", 1.5)
    l2, n2 = synth.baudot_bits(" " + M2, 1.5)
    level = np.concatenate([l1[:-1], [0, 1], l2])
    length = np.concatenate([n1[:-1], [3.0, 2.25], n2])
    return level.astype(np.uint8), length


def cases():
    out = [
        case("s85_45_15", M1, 0, 0, 1),
        case("s170_45_15", M1, 1, 0, 1),
        case("s200_50_1", M2, 2, 1, 0),
        case("s425_45_2", M2, 3, 0, 2),
        case("s450_50_15", M1, 4, 1, 1),
        case("s850_45_1", M1, 5, 0, 0),
        case("s170_50_2", M2, 1, 1, 2),
        case("s170_45_15_noatc", M1, 1, 0, 1, 1),
        case("s850_50_1_noatc", M2, 5, 1, 0, 1),
        case("s85_45_2_noatc", M2, 0, 0, 2, 1),
        case("figs_crlf", M3, 1, 0, 1),
        case("figs_crlf_noatc", M3, 3, 1, 0, 1),
        case("noisy", M1 + " " + M2, 1, 0, 1, noise_sigma=350.0, seed=3),
        case("noisy_noatc", M1 + " " + M2, 1, 0, 1, 1, verbatim=False, noise_sigma=700.0, seed=4),
        case("garbled", M1 + " " + M2, 1, 0, 1, verbatim=False, noise_sigma=2500.0, seed=7),
        case("garbled_noatc", M2 + " " + M1, 4, 1, 0, 1, verbatim=False, noise_sigma=2500.0, seed=8),
        case("fadeout", M1, 1, 0, 1, silence=14000),
        case("markfade", M2 + " " + M1 + " " + M2, 1, 0, 1, fade="mark", fade_depth=0.8, noise_sigma=20.0, seed=5),
        case("spacefade_noatc", M2 + " " + M1, 1, 0, 1, 1, verbatim=False, fade="space", fade_depth=0.9, noise_sigma=20.0, seed=6),
        case("badstop", M1 + " / " + M2, 1, 0, 1, verbatim=False, bits=broken_stop_bits()),
        case("silence", "", 1, 0, 1, verbatim=False, amplitude=0.0, lead=30000, tail=0),
        case("midchar", M1, 1, 0, 1, verbatim=False, lead=0, offset=700),
    ]
    return out


CHAIN_MSG = "RYRY CQ DE UHSDR K"
CHAIN_FRAMES = 128 * 2048          # 5.5 s: lead, up to 1 s of start offset, one pass and the start of the next


def chain_cases():
    """P48 DIGI at 170 Hz / 45.45 baud, and at 850 Hz / 50 baud with one stop bit"""
    return [
        dict(name="chain_p48_s170_45", path=48, shift_idx=1, speed_idx=0, stopbits_idx=1, atc_disable=0, channel=0),
        dict(name="chain_p48_s850_50", path=48, shift_idx=5, speed_idx=1, stopbits_idx=0, atc_disable=0, channel=1),
    ]


def chain_gen(c):
    return dict(channel=c["channel"], nframes=CHAIN_FRAMES, text=CHAIN_MSG, shift=synth.RTTY_SHIFTS[c["shift_idx"]],
                baud=synth.RTTY_SPEEDS[c["speed_idx"]], stopbits=synth.RTTY_STOPBITS[c["stopbits_idx"]], lead=4800)


def chain_iq(gen):
    g = dict(gen)
    return np.ascontiguousarray(synth.rtty_iq([g.pop("channel")], 0, g.pop("nframes"), g.pop("text"), **g)[0], dtype=np.int32)


def record_chain(out, writer, tmp):
    rec = os.path.join(out, "rtty_chain")
    for c in chain_cases():
        gen = chain_gen(c)
        iq = chain_iq(gen)
        fin, ftap, fchr = (os.path.join(tmp, c["name"] + x) for x in (".iq", ".tap", ".chr"))
        iq.tofile(fin)
        env = dict(os.environ, RTTY_SHIFT=str(c["shift_idx"]), RTTY_SPEED=str(c["speed_idx"]), RTTY_STOPBITS=str(c["stopbits_idx"]),
                   RTTY_ATC_DISABLE=str(c["atc_disable"]), RTTY_TAP_LOG=ftap, RTTY_CHAR_LOG=fchr)
        subprocess.run([rec, f"in={fin}", f"n={len(iq)}", "mode=6", f"path={c['path']}"], check=True, env=env)
        tap = np.fromfile(ftap, dtype=np.float32)
        assert len(tap) == len(iq) // 4, f"{c['name']}: {len(tap)} tap samples for {len(iq)} frames"
        res = open(fchr).read().split()
        char_sample = np.array(res[0::2], dtype=np.int32)
        chars = np.array(res[1::2], dtype=np.int64).astype(np.uint8)
        text = bytes(chars).decode("latin-1")
        print(f"{c['name']:18s} {len(iq):7d} frames   {text!r}")
        assert CHAIN_MSG in text, f"{c['name']}: the reference did not print the message verbatim"
        tap_crc = np.array([zlib.crc32(tap[k:k + 8].tobytes()) for k in range(0, len(tap), 8)], dtype=np.uint32)
        writer.save(f"rtty_{c['name']}.npz", gen=np.array(json.dumps(gen)), path=np.int32(c["path"]),
                    crc32=np.uint32(zlib.crc32(iq.tobytes())), tap_crc=tap_crc, tap_head=tap[:256].copy(),
                    shift_idx=np.int32(c["shift_idx"]), speed_idx=np.int32(c["speed_idx"]),
                    stopbits_idx=np.int32(c["stopbits_idx"]), atc_disable=np.int32(c["atc_disable"]), chars=chars,
                    char_sample=char_sample, message=np.array(CHAIN_MSG))


def audio_of(c):
    return synth.rtty_audio(c["bits"] if c["bits"] is not None else c["message"], **c["gen"])


def main():
    a = recording.parse_args()
    out = recording.build(a, ["rtty"], ["rtty", "rtty_chain"])
    drv = os.path.join(out, "rtty_driver")
    writer = recording.Recorder(a)

    resync = False
    with tempfile.TemporaryDirectory() as tmp:
        record_chain(out, writer, tmp)
        for c in cases():
            audio = audio_of(c)
            wav = os.path.join(tmp, c["name"] + ".f32")
            audio.tofile(wav)
            res = subprocess.run([drv, wav, str(c["shift_idx"]), str(c["speed_idx"]), str(c["stopbits_idx"]), str(c["atc_disable"])],
                                 check=True, capture_output=True, text=True).stdout.split()
            char_sample = np.array(res[0::2], dtype=np.int32)
            chars = np.array(res[1::2], dtype=np.int64).astype(np.uint8)
            text = bytes(chars).decode("latin-1")
            print(f"{c['name']:18s} {len(audio):7d} samples  {text!r}")
            if c["verbatim"]:
                assert c["message"] in text, f"{c['name']}: the reference did not print the message verbatim"
            if c["name"] == "badstop":
                assert M1 in text and M2 in text and (M1 + " E " + M2) not in text, "badstop: the broken character was printed"
                resync = True
            if c["name"] == "silence":
                assert len(chars) == 0
            bits = c["bits"] if c["bits"] is not None else (np.zeros(0, np.uint8), np.zeros(0))
            writer.save(f"rtty_{c['name']}.npz", gen=np.array(json.dumps(c["gen"])),
                        bits_level=bits[0], bits_length=bits[1], samples=np.int32(len(audio)),
                        crc32=np.uint32(zlib.crc32(audio.tobytes())), shift_idx=np.int32(c["shift_idx"]),
                        speed_idx=np.int32(c["speed_idx"]), stopbits_idx=np.int32(c["stopbits_idx"]),
                        atc_disable=np.int32(c["atc_disable"]), chars=chars, char_sample=char_sample,
                        message=np.array(c["message"]), verbatim=np.int32(bool(c["verbatim"])))
    assert resync
    writer.finish()


if __name__ == "__main__":
    main()
