#!/usr/bin/env python3
"""Record tests/golden/digimod_*.npz from the reference firmware's RTTY and BPSK modulators.

Builds tools/digimod/modgen_driver.c against the reference objects and its psk.c (digimod.mk,
through oracle/ref/Makefile) into a git-ignored or outside directory and runs every case of cases()
through it, one process per case (the modulators' statics never reset).  A case is a modulator, its
parameters, the queue's capacity and a list of ops: put text, generate n samples, StartTX /
PrepareTx.  Stored per case, data only:

  kind                       "rtty" or "psk"
  shift_idx, speed_idx, stopbits_idx, capacity
  ops json                   [["put", hex], ["gen", n], ["start"], ...]
  accepted int32 [puts]      what each put appended
  consumed uint32 [gens]     characters removed from the ring after each gen
  txoff_at uint32 [gens]     index of the first sample that requested TX-off, 0xffffffff: none
  state uint8 [gens]         Psk_Modulator_GetState after each gen (0 for RTTY)
  total int32                samples generated
  samples int16 [total]      the reference's GenSample results, for sequences up to 65536 samples
  block_crc uint32 [blocks]  else the crc32 of every block of 1024 samples (the last one shorter),
  window_at int32 [3], windows int16 [3][256]    and three windows of them raw

and, for the loopback (digimod_loop_*.npz, loop_cases()): the reference modulator's output, every
fourth sample as float, behind `lead` samples of silence through the reference decoder
(tools/rtty/rtty_driver.c, tools/psk/psk_driver.c):

  kind ... ops               as above
  message uint8 [k]          the text put
  leads int32 [m], lead      the leads tried in order and the one kept: the first at which the
  verbatim bool              reference printed the message; if none did, lead 0 and verbatim false
  chars uint8 [n]            the bytes the reference decoder printed at `lead`
  crc32                      of the modulator's int16 samples

A file whose recording has not changed is left as it is, so a re-recording reproduces the committed
files byte for byte; --check fails instead of writing where one would change.

  python3 tools/digimod/make_digimod_golden.py [--check] [--out DIR] [--ref /root/reference/mchf-eclipse]
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
WHOLE = 65536
BLOCK = 1024
WINDOW = 256


def put(text):
    return ["put", bytes(text).hex()]


def gen(n):
    return ["gen", int(n)]


START = ["start"]


def rtty(name, ops, shift=1, speed=0, stop=1, capacity=64):
    return dict(name="rtty_" + name, kind="rtty", shift_idx=shift, speed_idx=speed, stopbits_idx=stop, capacity=capacity, ops=ops)


def psk(name, ops, speed=0, capacity=64):
    return dict(name="psk_" + name, kind="psk", shift_idx=0, speed_idx=speed, stopbits_idx=0, capacity=capacity, ops=ops)


def cases():
    ch45 = 8 * 1056      # a character of 8 bits at 45.45 baud
    return [
        # 45.45 baud, 170 Hz at each stop-bit setting
        rtty("s170_45_1", [put(b"CQ DE K"), gen(WHOLE)], stop=0),
        rtty("s170_45_15", [put(b"RYRY CQ DE UHSDR K"), gen(200000)], stop=1),
        rtty("s170_45_2", [put(b"CQ DE K"), gen(WHOLE)], stop=2),
        rtty("s170_50", [put(b"THE QUICK BROWN FOX 0123456789"), gen(330000)], speed=1),
        # the narrowest and the widest shift: the waits for the tone change differ in length
        rtty("s85_45", [put(b"RYRYRY 599"), gen(120000)], shift=0),
        rtty("s850_45", [put(b"RYRYRY 599"), gen(120000)], shift=5),
        rtty("s425_50_1", [put(b"DE UHSDR"), gen(WHOLE)], shift=3, speed=1, stop=0),
        rtty("altfigs", [put(b"A1B2C3-D4?E5"), gen(230000)]),
        # lower case, bytes without a Baudot code, bytes above 0x7f (masked: 0xc1 is 'A', 0xe5 'e')
        rtty("lower_nocode", [put(b"abc%*<xyz\x00\x01\x7f\x80\xc1\xe5 ok\r\n\a'"), gen(260000)]),
        rtty("bytes", [put(bytes(range(128))), gen(900000)], speed=1, stop=0, capacity=160),
        rtty("idle", [gen(40000)]),
        # text after the start pair and three idle characters, in mid-character, into a queue of 8
        rtty("late_cap8", [gen(5 * ch45 + 1000), put(b"HELLO WORLD"), gen(70000), put(b"AGAIN"), gen(30000)], capacity=8),
        rtty("eot", [put(b"AB\x04CD\x04"), gen(90000)]),
        rtty("restart", [put(b"TEST"), gen(30000), START, gen(12345), START, gen(40000)]),
        # BPSK
        psk("31_text", [put(b"Hello de UHSDR"), gen(300000)], speed=0),
        psk("63_text", [put(b"CQ CQ de UHSDR, Pse k (QSL?) #7"), gen(330000)], speed=1),
        psk("125_text", [put(b"Test de DL1ABC: UR RST 599-579, QSL? Pwr 25W @ 14.070 MHz (73)!"), gen(330000)], speed=2, capacity=128),
        psk("31_idle", [gen(WHOLE)], speed=0),
        psk("125_idle", [gen(WHOLE)], speed=2),
        # every ASCII character; the EOT in its place adds 16 ones and the text behind it goes on
        psk("125_ascii", [put(bytes(range(128))), gen(700000)], speed=2, capacity=160),
        psk("125_high", [put(bytes(list(range(128, 256, 5)) + [255])), gen(220000)], speed=2),
        # EOT: postamble, INACTIVE, OFF, silence; then PrepareTx and more text
        psk("125_eot", [put(b"73 k\x04"), gen(150000), START, put(b"again"), gen(90000)], speed=2),
        psk("63_eot", [put(b"e\x04"), gen(140000)], speed=1),
        # the queue runs dry between characters; put in the middle of a bit
        psk("63_dry", [put(b"ab"), gen(100001), put(b"cd"), gen(40000), gen(20000)], speed=1),
        psk("31_cap8", [put(b"0123456789"), gen(200000), put(b"abcdefghij"), gen(150000)], speed=0, capacity=8),
    ]


def run_case(drv, c, tmp):
    fops, fout = os.path.join(tmp, c["name"] + ".ops"), os.path.join(tmp, c["name"] + ".s16")
    with open(fops, "w") as f:
        for op in c["ops"]:
            f.write(" ".join(str(x) for x in op) + "\n")
    args = [drv, "rtty", str(c["shift_idx"]), str(c["speed_idx"]), str(c["stopbits_idx"])] if c["kind"] == "rtty" else [drv, "psk", str(c["speed_idx"])]
    res = subprocess.run(args + [str(c["capacity"]), fops, fout], check=True, capture_output=True, text=True).stdout.splitlines()
    accepted = [int(x.split()[1]) for x in res if x.startswith("accepted")]
    gens = [[int(v) for v in x.split()[1:]] for x in res if x.startswith("gen")]
    samples = np.fromfile(fout, dtype=np.int16)
    total = sum(op[1] for op in c["ops"] if op[0] == "gen")
    assert len(samples) == total, f"{c['name']}: {len(samples)} samples for {total} asked"
    out = dict(kind=np.array(c["kind"]), shift_idx=np.int32(c["shift_idx"]), speed_idx=np.int32(c["speed_idx"]),
               stopbits_idx=np.int32(c["stopbits_idx"]), capacity=np.int32(c["capacity"]), ops=np.array(json.dumps(c["ops"])),
               accepted=np.array(accepted, np.int32), consumed=np.array([g[0] for g in gens], np.uint32),
               txoff_at=np.array([g[1] for g in gens], np.uint32), state=np.array([g[2] for g in gens], np.uint8),
               total=np.int32(total))
    if total <= WHOLE:
        out["samples"] = samples
    else:
        out["block_crc"] = np.array([zlib.crc32(samples[k:k + BLOCK].tobytes()) for k in range(0, total, BLOCK)], np.uint32)
        at = np.array([0, (total // 2) // BLOCK * BLOCK + 300, total - WINDOW], np.int32)
        out["window_at"] = at
        out["windows"] = np.stack([samples[k:k + WINDOW] for k in at])
    return out, samples


def loop_cases():
    """Modulator into decoder.  Both reference decoders sample on a fixed grid and the BPSK one has no
    timing recovery, so the 12 ksps audio is tried behind each of `leads` samples of silence, a few
    values across one symbol, and the first lead at which the reference prints the message is kept."""
    return [
        dict(name="loop_rtty_s170_45", mod=rtty("loop", [put(b"RYRY CQ DE UHSDR 599 K"), gen(300000)]), message=b"RYRY CQ DE UHSDR 599 K",
             leads=[0, 66, 132, 198]),
        dict(name="loop_psk_31", mod=psk("loop", [put(b"Hello de UHSDR k"), gen(400000)], speed=0), message=b"Hello de UHSDR k",
             leads=[0, 96, 192, 288]),
        dict(name="loop_psk_125", mod=psk("loop", [put(b"CQ CQ de UHSDR, 599 k"), gen(200000)], speed=2), message=b"CQ CQ de UHSDR, 599 k",
             leads=[0, 24, 48, 72]),
    ]


def decode(out, m, audio, tmp):
    """the bytes the reference decoder prints for 12 ksps float audio"""
    wav = os.path.join(tmp, "loop.f32")
    audio.astype(np.float32).tofile(wav)
    if m["kind"] == "rtty":
        args = [os.path.join(out, "rtty_driver"), wav, str(m["shift_idx"]), str(m["speed_idx"]), str(m["stopbits_idx"]), "0"]
    else:
        args = [os.path.join(out, "psk_driver"), wav, str(m["speed_idx"])]
    res = subprocess.run(args, check=True, capture_output=True, text=True).stdout.split()
    return np.array(res[1::2], dtype=np.int64).astype(np.uint8)


def record_loop(out, drv, c, tmp):
    """every fourth sample of the reference modulator's output, as float, through the reference decoder"""
    _, samples = run_case(drv, c["mod"], tmp)
    tried = []
    for lead in c["leads"]:
        chars = decode(out, c["mod"], np.concatenate([np.zeros(lead, np.float32), samples[::4].astype(np.float32)]), tmp)
        tried.append((lead, chars))
        if c["message"] in bytes(chars):
            break
    verbatim = c["message"] in bytes(tried[-1][1])
    lead, chars = tried[-1] if verbatim else tried[0]       # none: what lead 0 gave
    m = c["mod"]
    return dict(kind=np.array(m["kind"]), shift_idx=np.int32(m["shift_idx"]), speed_idx=np.int32(m["speed_idx"]),
                stopbits_idx=np.int32(m["stopbits_idx"]), capacity=np.int32(m["capacity"]), ops=np.array(json.dumps(m["ops"])),
                message=np.frombuffer(c["message"], np.uint8), leads=np.array(c["leads"], np.int32), lead=np.int32(lead),
                verbatim=np.bool_(verbatim), chars=chars, crc32=np.uint32(zlib.crc32(samples.tobytes())))


CHAIN_FRAMES = 98304        # 3072 calls of 32 frames


def chain_cases():
    """TxProcessor_Run in DIGI mode through the harness' main (tools/digimod/modtx_driver.c), 32-frame
    calls: USB and digi_lsb for each modulator, one run with the frequency translation switched on
    (which the DIGI branch must ignore) and with I/Q gains and a phase balance off their defaults"""
    return [
        dict(name="chain_rtty_usb", mod=rtty("chain", [put(b"RYRY DE UHSDR")]), args=dict(mode=6, path=48, iqmode=0, digilsb=0)),
        dict(name="chain_rtty_lsb_m12k", mod=rtty("chain", [put(b"CQ 599 73")], shift=5, speed=1, stop=0),
             args=dict(mode=6, path=48, iqmode=4, digilsb=1, txgi=1.03, txgq=0.98, txphase=0.02, txfilter=2)),
        dict(name="chain_psk_usb", mod=psk("chain", [put(b"CQ de UHSDR k")], speed=2), args=dict(mode=6, path=48, iqmode=0, digilsb=0)),
        dict(name="chain_psk_lsb", mod=psk("chain", [put(b"de UHSDR")], speed=0), args=dict(mode=6, path=48, iqmode=0, digilsb=1, txphase=-0.015)),
    ]


def record_chain(out, c, tmp):
    m, n = c["mod"], CHAIN_FRAMES
    fin, fiq, fa0, flog = (os.path.join(tmp, c["name"] + x) for x in (".in", ".iq", ".a0", ".log"))
    np.zeros((n, 2), np.int32).tofile(fin)          # the codec frames, which the DIGI branch never reads
    env = dict(os.environ, MODTX_KIND=m["kind"], MODTX_SHIFT=str(m["shift_idx"]), MODTX_SPEED=str(m["speed_idx"]),
               MODTX_STOP=str(m["stopbits_idx"]), MODTX_LSB=str(c["args"]["digilsb"]), MODTX_CAP=str(m["capacity"]),
               MODTX_TEXT=m["ops"][0][1], MODTX_LOG=flog)
    args = [f"{k}={v}" for k, v in c["args"].items() if k != "digilsb"]
    subprocess.run([os.path.join(out, "modtx_driver"), "tx=1", f"in={fin}", f"n={n}", f"out_dst={fiq}", f"out_a={fa0}", *args],
                   check=True, env=env)
    iq = np.fromfile(fiq, dtype=np.int32).reshape(n, 2)
    a0 = np.fromfile(fa0, dtype=np.float32)
    assert len(a0) == n and np.abs(iq).max() > 0
    consumed, txoff, state = (int(x) for x in open(flog).read().split())
    at = np.array([0, n // 2 + 300, n - WINDOW], np.int32)
    return dict(kind=np.array(m["kind"]), shift_idx=np.int32(m["shift_idx"]), speed_idx=np.int32(m["speed_idx"]),
                stopbits_idx=np.int32(m["stopbits_idx"]), capacity=np.int32(m["capacity"]), text=np.frombuffer(bytes.fromhex(m["ops"][0][1]), np.uint8),
                args=np.array(json.dumps(c["args"])), frames=np.int32(n),
                iq_crc=np.array([zlib.crc32(iq[k:k + 32].tobytes()) for k in range(0, n, 32)], np.uint32),
                a0_crc=np.array([zlib.crc32(a0[k:k + 32].tobytes()) for k in range(0, n, 32)], np.uint32),
                window_at=at, iq_win=np.stack([iq[k:k + WINDOW] for k in at]), a0_win=np.stack([a0[k:k + WINDOW] for k in at]),
                consumed=np.uint32(consumed), txoff=np.bool_(txoff != 0xffffffff), state=np.uint8(state))


def main():
    a = recording.parse_args()
    # the modulators' recorder, and the decoders' (tools/rtty, tools/psk) for the loopback
    out = recording.build(a, ["digimod", "rtty", "psk"], ["modgen_driver", "modtx_driver", "rtty", "psk_driver"])
    drv = os.path.join(out, "modgen_driver")
    writer = recording.Recorder(a)
    with tempfile.TemporaryDirectory() as tmp:
        for c in cases():
            rec, samples = run_case(drv, c, tmp)
            word = writer.save(f"digimod_{c['name']}.npz", **rec)
            print(f"{c['name']:18s} {len(samples):8d} samples  consumed {rec['consumed'][-1]:4d}  txoff {int(rec['txoff_at'][-1]):10d}  "
                  f"state {rec['state'][-1]}  accepted {rec['accepted'].tolist()}  peak {int(np.abs(samples.astype(np.int32)).max())}"
                  f"  {word}")
        for c in loop_cases():
            rec = record_loop(out, drv, c, tmp)
            word = writer.save(f"digimod_{c['name']}.npz", **rec)
            print(f"{c['name']:18s} lead {int(rec['lead']):4d}  verbatim {bool(rec['verbatim'])}  {bytes(rec['chars'])!r}  {word}")
        for c in chain_cases():
            rec = record_chain(out, c, tmp)
            word = writer.save(f"digimod_{c['name']}.npz", **rec)
            print(f"{c['name']:20s} consumed {int(rec['consumed']):3d}  state {int(rec['state'])}  peak iq {int(np.abs(rec['iq_win']).max())}"
                  f"  {word}")
    writer.finish()


if __name__ == "__main__":
    main()
