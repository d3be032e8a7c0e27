#!/usr/bin/env python3
"""Record tests/golden/cwgen_*.npz from the reference firmware's CW generator.

Builds tools/cwgen/cwgen_driver.c against the reference objects (cwgen.mk, through
oracle/ref/Makefile) into a git-ignored or outside directory and runs every case of cases() through
it, one process per case (the keyer's statics never reset).  A case is the keyer's settings, the text
queue's capacity and a list of ops: put text, set the speed, run `count` 32-sample blocks with the key
lines at a value.  Stored per case, data only:

  mode, speed, weight, reverse, rx_delay, sidetone, capacity
  ops json                   [["put", hex], ["speed", wpm, weight], ["blk", lines, count], ...]
  accepted int32 [puts]      what each put appended
  flags uint8 [B]            per block: bit 0 CwGen_Process returned true, bit 1 TX-on, bit 2 TX-off requested
  cw_state uint8 [B], key_timer int32 [B], sm_tbl_ptr uint8 [B], port_state uint8 [B], acc uint32 [B]
                             ps.* and the DDS accumulator after each block
  i_crc, q_crc uint32 [B]    crc32 of each block's 32 floats (zeros where the generator was silent)
  window_at int32 [3], i_win, q_win float32 [3][256]
                             three raw windows: over the first rising edge, the first and the last falling edge
  consumed uint32            characters removed from the ring or discarded by a key closure
  echo uint8 [k]             the bytes handed to UiDriver_TextMsgPutChar

for the transmit chain (cwgen_chain_*.npz, chain_cases(), TxProcessor_Run through tools/cwgen/cwtx_driver.c):
the keyer's settings, cw_lsb, text (put before the first call), keys uint8 [calls], the harness
arguments, flags uint8 [calls] (bit 0: the signal was active), a crc32 per 32-frame call of the int32
I/Q frames and of a_buffer[0], three raw windows of each, consumed and echo;

and cwgen_tables.npz: cw_char_codes / cw_char_chars / cw_sign_codes / cw_sign_chars and sm_table as
the compiled reference holds them (char_codes uint32, char_chars uint8, sign_codes uint32, sign_chars
uint8 [n][2], env float32 [128]); tools/cwgen/gen_cwgen_tables.py turns it into the library's table file.

A file whose recording has not changed is left as it is; --check fails instead of writing.

  python3 tools/cwgen/make_cwgen_golden.py [--check] [--out DIR] [--ref /root/reference/mchf-eclipse]
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
WINDOW = 256
IAM_B, IAM_A, STRAIGHT, ULTIMATE = range(4)
DIT, DAH, BOTH = 1, 2, 3


def put(text):
    return ["put", bytes(text).hex()]


def blk(lines, count):
    return ["blk", int(lines), int(count)]


def case(name, ops, mode=IAM_B, speed=48, weight=100, reverse=0, rx_delay=0, sidetone=750, capacity=32):
    return dict(name=name, mode=mode, speed=speed, weight=weight, reverse=reverse, rx_delay=rx_delay, sidetone=sidetone,
                capacity=capacity, ops=ops)


def times(speed, weight):
    """dit, dah, pause, space in blocks: only to size the gaps between gestures"""
    dit = 180000 // speed + 900
    corr = int((weight - 100) * dit / 100)
    return (dit + corr) // 100, (3 * 180000 // speed + 900 + corr) // 100, (180000 // speed - 900 - corr) // 100, 6 * 180000 // speed // 100


def gestures(idle=300):
    """at 48 wpm a dit is 46 blocks, a dah 121, the pause 28, the word space 225"""
    g = [
        [blk(DIT, 10)],                                     # single dit
        [blk(DAH, 10)],                                     # single dah
        [blk(DIT, 250)],                                    # held dit
        [blk(DAH, 400)],                                    # held dah
        [blk(DIT, 5), blk(BOTH, 400)],                      # squeeze from the dit side
        [blk(DAH, 5), blk(BOTH, 400)],                      # squeeze from the dah side
        [blk(DAH, 20), blk(0, 20), blk(DIT, 30)],           # a dit tapped during a dah's key-up
        [blk(BOTH, 60)],                                    # both released in the middle of an element
    ]
    return [op for x in g for op in x + [blk(0, idle)]]


def cases():
    out = [
        # straight key: one block's press still makes the whole rise, 8 blocks up and 8 down
        case("straight_tap", [blk(0, 5), blk(DAH, 1), blk(0, 40)], mode=STRAIGHT),
        case("straight_long", [blk(0, 3), blk(DAH, 200), blk(0, 150)], mode=STRAIGHT, rx_delay=2),
        # pressed again during the falling edge, and again while the break timer runs
        case("straight_repress", [blk(0, 2), blk(DAH, 30), blk(0, 4), blk(DAH, 20), blk(0, 30), blk(DAH, 15), blk(0, 80)],
             mode=STRAIGHT, rx_delay=1),
        case("straight_delay50", [blk(0, 2), blk(DAH, 20), blk(0, 2600)], mode=STRAIGHT, rx_delay=50, sidetone=600),
        # the DIT line and paddle_reverse mean nothing to the straight key; a closure empties the queue
        case("straight_reverse", [put(b"AB"), blk(0, 3), blk(DIT, 10), blk(0, 3), blk(DAH, 20), blk(0, 20)], mode=STRAIGHT, reverse=1),
        case("iam_a", gestures(), mode=IAM_A, rx_delay=3),
        case("iam_b", gestures(), mode=IAM_B, rx_delay=3),
        case("ultimate", gestures(), mode=ULTIMATE, rx_delay=3),
        case("iam_b_reverse", [blk(DIT, 10), blk(0, 300), blk(DAH, 10), blk(0, 300), blk(DIT, 5), blk(BOTH, 300), blk(0, 300)],
             mode=IAM_B, reverse=1),
        case("ultimate_reverse", [blk(DIT, 5), blk(BOTH, 300), blk(0, 300), blk(DAH, 5), blk(BOTH, 300), blk(0, 300)],
             mode=ULTIMATE, reverse=1),
    ]
    for speed in (5, 20, 48):
        for weight in (50, 100, 150):
            dit, dah, pause, space = times(speed, weight)
            out.append(case(f"timing_{speed}_{weight}", [blk(DIT, 5), blk(0, dit + pause + space + 50), blk(DAH, 5), blk(0, dah + pause + space + 50)],
                            mode=IAM_A, speed=speed, weight=weight, rx_delay=1))
    for tone in (400, 600, 750, 1000):
        out.append(case(f"tone_{tone}", [blk(DIT, 5), blk(0, 100), blk(DAH, 5), blk(0, 200)], sidetone=tone))
    out += [
        # lower case, a digit, punctuation, a character without a code (taken and dropped), one and two spaces
        case("text_sentence", [put(b"Ab 1,~  e?"), blk(0, 7000)]),
        case("text_mid_element", [put(b"A"), blk(0, 30), put(b"N"), blk(0, 1500)]),
        case("text_full", [put(b"EEEEEEEEEEEE"), blk(0, 1200), put(b"TI"), blk(0, 1800)], capacity=8),
        # a paddle closes while text is sent: the queue is emptied
        case("text_paddle", [put(b"TTTT"), blk(0, 200), blk(DIT, 10), blk(0, 800)]),
        # what CwGen_AddChar prints: a keyed A, <AR>, six dits (no such code), nine dahs (cw_char above 50000)
        case("echo", [blk(DIT, 40), blk(0, 10), blk(DAH, 40), blk(0, 600), blk(BOTH, 460), blk(0, 600), blk(DIT, 390), blk(0, 600),
                      blk(DAH, 1212), blk(0, 700)], mode=IAM_A),
        case("set_speed", [put(b"K"), blk(0, 100), ["speed", 48, 120], blk(0, 1500)], speed=30),
    ]
    return out


def windows_at(active, total):
    """sample indices of three windows: the first rising edge, the first and the last falling edge"""
    a = active.astype(np.int8)
    up = np.flatnonzero(np.diff(a) > 0) + 1
    down = np.flatnonzero(np.diff(a) < 0) + 1
    at = [32 * (int(up[0]) - 1) if len(up) else 0,
          32 * (int(down[0]) - 7) if len(down) else total // 2,
          32 * (int(down[-1]) - 7) if len(down) else total - WINDOW]
    return np.clip(np.array(at, np.int32), 0, max(total - WINDOW, 0))


def run_case(drv, c, tmp):
    fops, fout = os.path.join(tmp, c["name"] + ".ops"), os.path.join(tmp, c["name"] + ".bin")
    with open(fops, "w") as f:
        for op in c["ops"]:
            f.write(" ".join(str(x) for x in op) + "\n")
    args = [drv, "gen"] + [str(c[k]) for k in ("mode", "speed", "weight", "reverse", "rx_delay", "sidetone", "capacity")]
    res = subprocess.run(args + [fops, fout], check=True, capture_output=True, text=True).stdout.splitlines()
    accepted = [int(x.split()[1]) for x in res if x.startswith("accepted")]
    end = [x.split() for x in res if x.startswith("end")][0]
    blocks = sum(op[2] for op in c["ops"] if op[0] == "blk")
    rec = np.fromfile(fout, dtype=np.uint32).reshape(blocks, 6 + 64)
    ints, iq = rec[:, :6], rec[:, 6:].view(np.float32).reshape(blocks, 2, 32)
    i, q = np.ascontiguousarray(iq[:, 0]).reshape(-1), np.ascontiguousarray(iq[:, 1]).reshape(-1)
    at = windows_at(ints[:, 0] & 1, 32 * blocks)
    assert blocks * 32 >= WINDOW
    out = dict({k: np.int32(c[k]) for k in ("mode", "speed", "weight", "reverse", "rx_delay", "sidetone", "capacity")},
               ops=np.array(json.dumps(c["ops"])), accepted=np.array(accepted, np.int32),
               flags=ints[:, 0].astype(np.uint8), cw_state=ints[:, 1].astype(np.uint8), key_timer=ints[:, 2].astype(np.int32),
               sm_tbl_ptr=ints[:, 3].astype(np.uint8), port_state=ints[:, 4].astype(np.uint8), acc=ints[:, 5].copy(),
               i_crc=np.array([zlib.crc32(i[k:k + 32].tobytes()) for k in range(0, len(i), 32)], np.uint32),
               q_crc=np.array([zlib.crc32(q[k:k + 32].tobytes()) for k in range(0, len(q), 32)], np.uint32),
               window_at=at, i_win=np.stack([i[k:k + WINDOW] for k in at]), q_win=np.stack([q[k:k + WINDOW] for k in at]),
               consumed=np.uint32(int(end[1])), echo=np.frombuffer(bytes.fromhex(end[2] if len(end) > 2 else ""), np.uint8))
    assert (ints[:, 1:5] < 2 ** 31).all() and ints[:, 3].max() <= 128
    return out


CHAIN_FRAMES = 49152       # 1536 calls of 32 frames


def chain_cases():
    """TxProcessor_Run in CW mode through the harness' main (tools/cwgen/cwtx_driver.c), 32-frame
    calls: keys is a list of [lines, calls] runs, padded with open lines to CHAIN_FRAMES / 32 calls"""
    return [
        dict(name="chain_usb_text", keyer=case("", [], mode=IAM_B, rx_delay=1), text=b"Cq 5", keys=[], lsb=0, args=dict(mode=2, iqmode=4)),
        dict(name="chain_lsb_straight", keyer=case("", [], mode=STRAIGHT, rx_delay=2, sidetone=600), text=b"",
             keys=[[0, 5], [DAH, 1], [0, 40], [DAH, 200], [0, 150], [DAH, 30], [0, 4], [DAH, 20]], lsb=1, args=dict(mode=2, iqmode=0)),
        dict(name="chain_gains", keyer=case("", [], mode=IAM_A, rx_delay=1), text=b"", keys=[[DIT, 40], [0, 10], [DAH, 40], [0, 400], [BOTH, 460]], lsb=0,
             args=dict(mode=2, iqmode=0, txgi=1.03, txgq=0.98, txphase=0.02, txpwr=0.37)),
        dict(name="chain_tune", keyer=case("", [], mode=STRAIGHT, rx_delay=1, sidetone=1000), text=b"",
             keys=[[0, 3], [DAH, 30], [0, 287], [0, 192], [DAH, 40]], lsb=0, args=dict(mode=2, iqmode=4, txphase=-0.015, tune="320:192:1")),
    ]


def record_chain(out, c, tmp):
    k, n = c["keyer"], CHAIN_FRAMES
    keys = np.zeros(n // 32, np.uint8)
    b = 0
    for lines, count in c["keys"]:
        keys[b:b + count] = lines
        b += count
    fin, fiq, fa0, flog, fkeys, fflags = (os.path.join(tmp, c["name"] + x) for x in (".in", ".iq", ".a0", ".log", ".keys", ".flags"))
    np.zeros((n, 2), np.int32).tofile(fin)          # the codec frames, which the CW branch never reads
    keys.tofile(fkeys)
    env = dict(os.environ, CWTX_MODE=str(k["mode"]), CWTX_SPEED=str(k["speed"]), CWTX_WEIGHT=str(k["weight"]), CWTX_REVERSE=str(k["reverse"]),
               CWTX_RXDELAY=str(k["rx_delay"]), CWTX_SIDETONE=str(k["sidetone"]), CWTX_LSB=str(c["lsb"]), CWTX_CAP=str(k["capacity"]),
               CWTX_TEXT=c["text"].hex(), CWTX_KEYS=fkeys, CWTX_LOG=flog, CWTX_FLAGS=fflags)
    subprocess.run([os.path.join(out, "cwtx_driver"), "tx=1", f"in={fin}", f"n={n}", f"out_dst={fiq}", f"out_a={fa0}",
                    *[f"{a}={v}" for a, v in c["args"].items()]], check=True, env=env)
    iq = np.fromfile(fiq, dtype=np.int32).reshape(n, 2)
    a0 = np.fromfile(fa0, dtype=np.float32)
    flags = np.fromfile(fflags, dtype=np.uint8)
    assert len(a0) == n and len(flags) == n // 32 and np.abs(iq).max() > 0, (c["name"], len(a0), len(flags), int(np.abs(iq).max()))
    consumed, *echo = open(flog).read().split()
    at = windows_at(flags & 1, n)
    return dict({x: np.int32(k[x]) for x in ("mode", "speed", "weight", "reverse", "rx_delay", "sidetone", "capacity")}, cw_lsb=np.int32(c["lsb"]),
                text=np.frombuffer(c["text"], np.uint8), keys=keys, args=np.array(json.dumps(c["args"])), frames=np.int32(n), flags=flags,
                iq_crc=np.array([zlib.crc32(iq[j:j + 32].tobytes()) for j in range(0, n, 32)], np.uint32),
                a0_crc=np.array([zlib.crc32(a0[j:j + 32].tobytes()) for j in range(0, n, 32)], np.uint32),
                window_at=at, iq_win=np.stack([iq[j:j + WINDOW] for j in at]), a0_win=np.stack([a0[j:j + WINDOW] for j in at]),
                consumed=np.uint32(int(consumed)), echo=np.frombuffer(bytes.fromhex(echo[0] if echo else ""), np.uint8))


def record_tables(drv, tmp):
    sizes = {}
    for line in subprocess.run(["nm", "-S", drv], check=True, capture_output=True, text=True).stdout.splitlines():
        f = line.split()
        if len(f) == 4 and f[3] in ("cw_char_codes", "cw_char_chars", "cw_sign_codes", "cw_sign_chars"):
            sizes[f[3]] = int(f[1], 16)
    nchars, nsigns = sizes["cw_char_chars"], sizes["cw_sign_codes"] // 4
    assert sizes["cw_char_codes"] == 4 * nchars and sizes["cw_sign_chars"] == 8 * nsigns
    path = os.path.join(tmp, "tables.bin")
    subprocess.run([drv, "tables", str(nchars), str(nsigns), path], check=True)
    raw = open(path, "rb").read()
    assert np.frombuffer(raw[:8], np.uint32).tolist() == [nchars, nsigns]
    o = 8
    char_codes = np.frombuffer(raw, np.uint32, nchars, o); o += 4 * nchars
    char_chars = np.frombuffer(raw, np.uint8, nchars, o); o += nchars
    sign_codes = np.frombuffer(raw, np.uint32, nsigns, o); o += 4 * nsigns
    sign_chars = np.frombuffer(raw, np.uint8, 2 * nsigns, o).reshape(nsigns, 2); o += 2 * nsigns
    env = np.frombuffer(raw, np.float32, 128, o)
    assert o + 512 == len(raw)
    return dict(char_codes=char_codes, char_chars=char_chars, sign_codes=sign_codes, sign_chars=sign_chars, env=env)


def main():
    a = recording.parse_args()
    out = recording.build(a, ["cwgen"], ["cwgen_driver", "cwtx_driver"])
    drv = os.path.join(out, "cwgen_driver")
    writer = recording.Recorder(a)
    with tempfile.TemporaryDirectory() as tmp:
        recs = [("tables", record_tables(drv, tmp))] + [(c["name"], run_case(drv, c, tmp)) for c in cases()]
        recs += [(c["name"], record_chain(out, c, tmp)) for c in chain_cases()]
        for name, rec in recs:
            word = writer.save(f"cwgen_{name}.npz", **rec)
            if name == "tables":
                print(f"tables: {len(rec['char_codes'])} characters, {len(rec['sign_codes'])} prosigns  {word}")
            elif name.startswith("chain_"):
                print(f"{name:18s} {len(rec['flags']):6d} calls  {int((rec['flags'] & 1).sum()):5d} active  consumed {int(rec['consumed']):3d}  "
                      f"echo {bytes(rec['echo'])!r}  peak iq {int(np.abs(rec['iq_win']).max())}  {word}")
            else:
                print(f"{name:18s} {len(rec['flags']):6d} blocks  {int((rec['flags'] & 1).sum()):5d} with a tone  consumed {int(rec['consumed']):3d}  "
                      f"accepted {rec['accepted'].tolist()}  echo {bytes(rec['echo'])!r}  {word}")
    writer.finish()


if __name__ == "__main__":
    main()
