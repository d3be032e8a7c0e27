#!/usr/bin/env python3
"""Record the waterfall-image fixtures (tests/golden/wfall_*.npz) from the reference firmware.

Builds tools/wfall/wfall_driver.c with wfall_spectrum_tu.c against the reference objects (wfall.mk,
through oracle/ref/Makefile), runs one process per case and channel (the ring, the counters and
doubleLineStart are globals and statics) and records per case:

  wfall_<case>.npz   the configuration; lines u8 [C][F][W] and center_hz u32 [C][F] as the frames
                     brought them (for the case behind a spectrum recording: the bytes
                     UiSpectrum_DrawWaterfall itself formed from the harness' averages); per channel
                     and frame `drawn` and, where the frame drew, the image u16 [H][W] in the order of
                     the UiLcdHy28_BulkPixel_PutBuffer calls (zeros where it did not draw); `at`, the
                     ring line each frame wrote; and what the firmware computed: wfall_size, repeat,
                     marker_num, hz_per_pixel, rx_carrier_pos, marker_pos[3], the 65 colours, and
                     sd.wfall_line / sd.wfall_line_update after the last frame
  wfall_tables.npz   the five palettes of waterfall_colours.h

The maker asserts what the set must show (tools/README.md); tests/wfall_cases.py asserts it again on
load.  A recording that has not changed leaves its file alone; --check fails where one would change.

  python3 tools/wfall/make_wfall_golden.py [--out DIR] [--ref DIR] [--check]
"""
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recording  # noqa: E402

FIELDS = ("width", "height", "color_scheme", "vert_step_size", "marker_colour", "magnify", "iq_freq_mode", "dmod_mode", "digital_mode",
          "cw_lsb", "digi_lsb", "cw_sidetone_freq", "rtty_shift_idx", "psk_speed_idx", "tx_minus_rx_hz")
MARKER = 0xF81F          # magenta: in none of the palettes
DEFAULT = dict(width=128, height=4, color_scheme=0, vert_step_size=1, marker_colour=MARKER, magnify=0, iq_freq_mode=4, dmod_mode=0,
               digital_mode=0, cw_lsb=0, digi_lsb=0, cw_sidetone_freq=750, rtty_shift_idx=1, psk_speed_idx=0, tx_minus_rx_hz=0)
CW, DIGI = 2, 6          # UHSDR_DEMOD_*
MAX_BYTES = 977777       # the largest fixture of tests/golden before this module
SPEC = "p48_usb_256"     # the spectrum recording behind the chained case
SPEC_DISPLAY = dict(fft_len=256, width=256, spectrum_db_scale=3, spectrum_agc_rate=25, waterfall_contrast=120)


def ramp(C, F, W, lo=1):
    """lines that differ from frame to frame and channel to channel, bytes lo .. 63"""
    c, f, x = np.meshgrid(np.arange(C), np.arange(F), np.arange(W), indexing="ij")
    return ((x * 3 + f * 5 + c * 11) % (64 - lo) + lo).astype(np.uint8)


def hz_per_pixel(cfg):
    return np.float32(48000.0) / np.float32((1 << cfg["magnify"]) * cfg["width"])


def alternating(cfg, C, steps):
    """centre frequencies per ring line: base, base + d0, base, base + d1, ...: a drawing at base sees the
    lines at +d, one at base + d sees the base lines at -d.  With repeat 1 frame 0 has a ring line of its own and
    then every two frames share one."""
    F = 1 + 4 * len(steps)
    hz = np.zeros((C, F), np.uint64)
    for c in range(C):
        base = (7100000, 2 ** 32 - 50, 100)[c]         # channels 1 and 2 wrap the uint32 in one direction each
        order = steps if c == 0 else [-d for d in steps][::-1] if c == 1 else steps[::-1]
        for f in range(F):
            j = (f + 1) // 2
            hz[c, f] = (base + (order[j // 2] if j % 2 else 0)) % 2 ** 32
    return hz.astype(np.uint32)


def shift_steps(cfg):
    """in Hz: 0, one pixel exactly (or just past it where a pixel is no whole number of Hz), fractions of a pixel,
    several pixels, width - 1 pixels, and width pixels and more"""
    h, W = float(hz_per_pixel(cfg)), cfg["width"]
    up = lambda v: int(np.ceil(v))           # noqa: E731
    return [0, up(h), int(0.6 * h), up(1.6 * h), up(5 * h), up(17.3 * h), up((W - 1) * h), up(W * h), up((W + 40) * h), up(3 * W * h)]


def cases():
    """name -> (config, lines [C][F][W], center_hz [C][F] or None)"""
    out = {}
    for k in range(5):
        cfg = dict(DEFAULT, color_scheme=k)
        out[f"pal{k}"] = (cfg, ramp(2, 6, 128, lo=0), None)
    # bytes 64 (the marker's entry) and 255 (behind the palette): the firmware reads sd.waterfall_colours[255]
    # from bytes 379 and 380 of its own ring, so columns 123 and 124 of ring line 2 (width 128) stay 0 and the palette
    # is the grey one, whose entry 0 is 0: what it reads there is then colour 0, which is what the library defines
    lines = ramp(2, 12, 128)
    lines[:, :, 5::9] = 64
    lines[:, :, 7::13] = 255
    lines[:, :, 120:] = 0
    out["above"] = (dict(DEFAULT), lines, None)
    out["step2"] = (dict(DEFAULT, height=5, vert_step_size=2, color_scheme=2), ramp(3, 13, 128), None)
    out["step5"] = (dict(DEFAULT, height=5, vert_step_size=5, color_scheme=3), ramp(2, 14, 128), None)
    out["wrap"] = (dict(DEFAULT, height=3, color_scheme=1), ramp(2, 15, 128), None)               # 15 frames around a ring of 3
    out["w200_h9"] = (dict(DEFAULT, width=200, height=9, color_scheme=4), ramp(2, 7, 200), None)
    out["repeat2_odd"] = (dict(DEFAULT, width=256, height=81, color_scheme=2), ramp(1, 7, 256), None)   # 20736 bytes: halved to 40 lines
    out["memlimit"] = (dict(DEFAULT, width=480, height=87, color_scheme=1, vert_step_size=2), ramp(1, 6, 480), None)     # 20480 / 480 = 42 lines
    panel = dict(DEFAULT, width=480, height=70, color_scheme=3, magnify=1)
    out["panel"] = (panel, ramp(1, 5, 480), np.array([[7100000, 7100000, 7100350, 7100350, 7099000]], np.uint32))
    for m in range(6):
        cfg = dict(DEFAULT, height=9, color_scheme=2, magnify=m)
        hz = alternating(cfg, 3, shift_steps(cfg))
        out[f"shift_m{m}"] = (cfg, ramp(3, hz.shape[1], 128), hz)
    # every older line at least a width below, then above, the frame that draws
    for name, sign in (("far_below", 1), ("far_above", -1)):
        cfg = dict(DEFAULT, height=7, color_scheme=2)
        F = 9
        hz = (2 ** 31 + sign * ((np.arange(F, dtype=np.int64) + 1) // 2) * (48000 + 375 * 3))[None, :].repeat(2, 0)
        out[name] = (cfg, ramp(2, F, 128), (hz % 2 ** 32).astype(np.uint32))
    mk = dict(DEFAULT, width=200, height=3, color_scheme=2)
    out["mk_cw_usb"] = (dict(mk, dmod_mode=CW, cw_sidetone_freq=750, iq_freq_mode=4), ramp(1, 3, 200), None)
    out["mk_cw_lsb"] = (dict(mk, dmod_mode=CW, cw_lsb=1, cw_sidetone_freq=600, magnify=1, iq_freq_mode=1), ramp(1, 3, 200), None)
    out["mk_rtty"] = (dict(mk, dmod_mode=DIGI, digital_mode=1, rtty_shift_idx=5, iq_freq_mode=1), ramp(1, 3, 200), None)
    out["mk_rtty_lsb"] = (dict(mk, dmod_mode=DIGI, digital_mode=1, rtty_shift_idx=3, digi_lsb=1, iq_freq_mode=2, magnify=2), ramp(1, 3, 200), None)
    out["mk_bpsk"] = (dict(mk, dmod_mode=DIGI, digital_mode=2, psk_speed_idx=2, digi_lsb=1, magnify=3, iq_freq_mode=3), ramp(1, 3, 200), None)
    out["mk_bpsk_usb"] = (dict(mk, dmod_mode=DIGI, digital_mode=2, psk_speed_idx=0, magnify=5), ramp(1, 3, 200), None)
    out["mk_default"] = (dict(mk, iq_freq_mode=0), ramp(1, 3, 200), None)
    out["mk_digi_none"] = (dict(mk, dmod_mode=DIGI, digital_mode=0, iq_freq_mode=3), ramp(1, 3, 200), None)
    out["mk_off_right"] = (dict(mk, dmod_mode=CW, tx_minus_rx_hz=100000), ramp(1, 3, 200), None)
    out["mk_tx_shift"] = (dict(mk, dmod_mode=CW, tx_minus_rx_hz=-5000, iq_freq_mode=0), ramp(1, 3, 200), None)
    out["mk_negative"] = (dict(mk, dmod_mode=CW, tx_minus_rx_hz=-100000, iq_freq_mode=0), ramp(1, 3, 200), None)
    # a negative position whose low 16 bits are a column: -65533.33 + 99.5 + 3.125 -> -65430 -> 106
    out["mk_negative_low_bits"] = (dict(mk, dmod_mode=CW, tx_minus_rx_hz=-15728000, iq_freq_mode=0), ramp(1, 3, 200), None)
    return out


def parse(raw, F, W, H):
    """the driver's out.bin: (center_hz [F], at [F], lines [F][W], drawn [F], image [F][H][W], tail)"""
    hz, at, lines = np.zeros(F, np.uint32), np.zeros(F, np.int32), np.zeros((F, W), np.uint8)
    drawn, image = np.zeros(F, np.uint8), np.zeros((F, H, W), np.uint16)
    o = 0
    for f in range(F):
        hz[f], at[f] = struct.unpack_from("<Ii", raw, o)
        lines[f] = np.frombuffer(raw, np.uint8, W, o + 8)
        put = struct.unpack_from("<i", raw, o + 8 + W)[0]
        o += 12 + W
        assert put in (0, H), put
        if put:
            drawn[f] = 1
            image[f] = np.frombuffer(raw, np.uint16, H * W, o).reshape(H, W)
            o += 2 * H * W
    assert len(raw) - o == 12 + 20 + 132 + 20, (len(raw), o)
    tail = dict(ints=np.frombuffer(raw, np.int32, 3, o).copy(), floats=np.frombuffer(raw, np.float32, 5, o + 12).copy(),
                colours=np.frombuffer(raw, np.uint16, 65, o + 32).copy(), echo=np.frombuffer(raw, np.int32, 5, o + 164).copy())
    return hz, at, lines, drawn, image, tail


def collect(per_channel, name):
    """[(hz, at, lines, drawn, image, tail)] per channel -> the recording's arrays; the counters and the plan are every channel's"""
    first = per_channel[0]
    for other in per_channel[1:]:
        assert (other[1] == first[1]).all() and (other[3] == first[3]).all(), name
        assert all(other[5][k].tobytes() == first[5][k].tobytes() for k in first[5]), name
    tail = first[5]
    return dict(center_hz=np.stack([p[0] for p in per_channel]), at=first[1], lines=np.stack([p[2] for p in per_channel]),
                drawn=np.stack([p[3] for p in per_channel]), image=np.stack([p[4] for p in per_channel]), plan_ints=tail["ints"],
                plan_floats=tail["floats"], colours=tail["colours"], counters=tail["echo"][3:].copy()), tail["echo"]


def run(driver, tmp, cfg, lines, center_hz):
    C, F, W = lines.shape
    fin, fout = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    got = []
    for c in range(C):
        with open(fin, "wb") as f:
            f.write(struct.pack("<16i", *(cfg[k] for k in FIELDS), F))
            for k in range(F):
                f.write(struct.pack("<I", int(center_hz[c, k]) if center_hz is not None else 0) + lines[c, k].tobytes())
        subprocess.run([driver, "run", fin, fout], check=True)
        got.append(parse(open(fout, "rb").read(), F, W, cfg["height"]))
        assert (got[-1][2] == lines[c]).all(), "the ring does not hold the bytes the frames brought"
    return got


def run_spec(driver, tmp, golden, cfg):
    """the harness' spectrum run of the recording's I/Q with states 4 and 5 behind every frame, the first two channels"""
    with np.load(os.path.join(golden, f"spec_{SPEC}.npz")) as z:
        iq, avg, args = z["iq"], z["avg"], json.loads(str(z["args"]))
    C, F, L = 2, avg.shape[1], avg.shape[2]
    d = SPEC_DISPLAY
    assert L == d["fft_len"]
    fin, fout, fm, fa = (os.path.join(tmp, x) for x in ("iq.bin", "out.bin", "m.bin", "a.bin"))
    got = []
    for c in range(C):
        iq[c].astype(np.int32).tofile(fin)
        subprocess.run([driver, "spec", fout, str(L), str(cfg["width"]), str(d["spectrum_db_scale"]), str(d["spectrum_agc_rate"]),
                        str(d["waterfall_contrast"]), str(cfg["height"]), str(cfg["color_scheme"]), str(cfg["vert_step_size"]),
                        str(cfg["marker_colour"]), f"in={fin}", f"n={iq.shape[1]}", f"out_mag={fm}", f"out_avg={fa}",
                        *(f"{k}={v}" for k, v in args.items())], check=True)
        assert np.fromfile(fa, np.float32)[:F * L].tobytes() == avg[c].tobytes(), "the run is not the recording's"
        got.append(parse(open(fout, "rb").read(), F, cfg["width"], cfg["height"]))
    return got


def head_run(image):
    """how many rows from the top equal row 0"""
    n = 1
    while n < len(image) and (image[n] == image[0]).all():
        n += 1
    return n


def main():
    a = recording.parse_args()
    out = recording.build(a, ["wfall"], ["wfall_driver"])
    writer = recording.Recorder(a)
    driver = os.path.join(out, "wfall_driver")
    reached = {k: set() for k in range(5)}
    left = right = 0
    quirk = {}
    heads, idle = set(), 0

    with tempfile.TemporaryDirectory() as tmp:
        tab = os.path.join(tmp, "tables.bin")
        subprocess.run([driver, "tables", tab], check=True)
        raw = open(tab, "rb").read()
        assert struct.unpack("<i", raw[:4])[0] == 5
        palettes = np.frombuffer(raw[4:], np.uint16).reshape(5, 64).copy()
        assert not (palettes == MARKER).any() and (palettes[2, 1:] != 0).all() and palettes[0, 0] == 0
        print("tables", writer.save("wfall_tables.npz", palettes=palettes))

        todo = cases()
        todo[f"spec_{SPEC}"] = (dict(DEFAULT, width=256, height=7, color_scheme=1), None, None)
        for name, (cfg, lines, center_hz) in todo.items():
            extra = {}
            if lines is None:
                got = run_spec(driver, tmp, a.golden, cfg)
                extra = dict(spec=np.array(SPEC), display=np.array(json.dumps(SPEC_DISPLAY)))
            else:
                got = run(driver, tmp, cfg, lines, center_hz)
            rec, echo = collect(got, name)
            cfg = dict(cfg, magnify=int(echo[0]), iq_freq_mode=int(echo[1]), dmod_mode=int(echo[2]))     # as the firmware had them
            C, F, W = rec["lines"].shape
            H = cfg["height"]
            size, repeat, markers = (int(v) for v in rec["plan_ints"])
            assert 1 <= C <= 3 and size <= 80, name
            assert (rec["colours"][:64] == palettes[cfg["color_scheme"]]).all() and rec["colours"][64] == cfg["marker_colour"], name
            img, drawn = rec["image"], rec["drawn"].astype(bool)
            reached[cfg["color_scheme"]] |= set(img[drawn].ravel().tolist())
            idle += int((~drawn).sum())
            rows = img[drawn].reshape(-1, W)
            body = (rows != 0) & (rows != cfg["marker_colour"])
            left += int((~body[:, 0] & body[:, -1]).sum())
            right += int((body[:, 0] & ~body[:, -1]).sum())
            only_last = int((~body[:, :-1].any(axis=1) & body[:, -1]).sum())
            if name in ("far_below", "far_above"):
                quirk[name] = only_last
                # every row but those of the newest line is the quirk's: nothing of the other padding
                assert int((body[:, 0] & ~body[:, -1]).sum()) == 0, name
            if name == "w200_h9":
                heads |= {head_run(img[c, f]) for c in range(C) for f in range(F) if drawn[c, f]}
            if name == "panel":
                assert (size, repeat) == (35, 2), name
            if name == "memlimit":
                assert size == 20480 // W and size < H // 2, name
            if name == "repeat2_odd":
                assert (size, repeat) == (H // 2, 2) and H % 2 == 1, name
            if name == "wrap":
                assert F > 2 * size, name
            on_screen = int((img[0, np.flatnonzero(drawn[0])[0], 0] == cfg["marker_colour"]).sum())
            if name in ("mk_rtty", "mk_rtty_lsb", "mk_bpsk", "mk_bpsk_usb"):
                assert markers == 2 and on_screen == 2, (name, on_screen)
            if name in ("mk_off_right", "mk_negative"):
                assert markers == 1 and on_screen == 0, (name, on_screen)
            if name == "mk_negative_low_bits":
                assert rec["plan_floats"][2] < -65000 and on_screen == 1, (name, rec["plan_floats"])
            if name == "above":
                at64, at255 = rec["lines"] == 64, rec["lines"] == 255
                assert at64.any() and at255.any() and (rec["lines"][:, :, 123:125] == 0).all(), name
            word = writer.save(f"wfall_{name}.npz", config=np.array(json.dumps(cfg)), **rec, **extra)
            path = os.path.join(a.golden, f"wfall_{name}.npz")
            assert not os.path.exists(path) or os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
            print(f"{name:22s} C {C} F {F:2d} {W} x {H:2d} size {size:2d} repeat {repeat} markers {markers} at {rec['plan_floats'][2:2 + markers]} "
                  f"drawings {int(drawn.sum()):3d}", word)
    for k in range(5):
        assert set(palettes[k].tolist()) <= reached[k], (k, sorted(set(palettes[k].tolist()) - reached[k]))
    assert left > 0 and right > 0, (left, right)
    assert quirk["far_below"] > 0 and quirk["far_above"] > 0, quirk
    assert idle > 0
    assert heads == {1, 2}, heads
    writer.finish()


if __name__ == "__main__":
    main()
