#!/usr/bin/env python3
"""Record the display-stage fixtures (tests/golden/display_*.npz) from the reference firmware.

Builds tools/display/display_driver.c with display_spectrum_tu.c against the reference objects
(display.mk, through oracle/ref/Makefile), runs one process per case and channel (sd.display_offset
is a global) and records per case:

  display_<case>.npz   the configuration, where the frames of sd.FFT_AVGData come from (a spectrum
                       recording tests/golden/spec_*.npz, or the frames themselves for a synthetic
                       case) with their crc32, `edge` per channel and frame (what sd.FFT_Samples[fft_len]
                       held: for a spectrum recording float fft_len of the reference's own arm_cfft_f32
                       stages on that frame's ring snapshot), and per channel and frame the heights of
                       UiSpectrum_DrawScope, the byte line of UiSpectrum_DrawWaterfall,
                       sd.display_offset after the frame and min1; sd.db_scale, sd.agc_rate and
                       sd.wfall_contrast as UiSpectrum_InitSpectrumDisplayData left them; and
                       reads_edge: whether another sd.FFT_Samples[fft_len] changes the last column
  display_tables.npz   scope_scaling_factors[].value

For a spectrum recording the run is the harness' own (receive path, ring, window, transform,
magnitude, average), and its magnitude and average must equal the recording's bytes.  The maker
asserts what the set must show (tests/display_cases.py asserts it again on load).  A recording that
has not changed leaves its file alone; --check fails where one would change.

  python3 tools/display/make_display_golden.py [--out DIR] [--ref DIR] [--check]
"""
import json
import os
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recording  # noqa: E402

FIELDS = ("fft_len", "width", "spectrum_db_scale", "spectrum_agc_rate", "waterfall_contrast", "scope_h")
DEFAULT = dict(fft_len=256, width=0, spectrum_db_scale=3, spectrum_agc_rate=25, waterfall_contrast=120, scope_h=0)
SPECS = ("p48_usb_256", "p48_usb_512", "p48_zoom2_256", "p48_zoom8_512_iqauto")
OUTPUTS = ("scope", "wfall", "offset", "min")


def resolved(cfg):
    """width and scope_h 0 as the firmware's panels have them"""
    L = cfg["fft_len"]
    return dict(cfg, width=cfg["width"] or (256 if L == 256 else 480), scope_h=cfg["scope_h"] or (21 if L == 256 else 64))


def spectrum(rng, C, F, L, level, peaks=3):
    """averages as state 3 leaves them (never below 1): a noise floor per channel and a few carriers"""
    avg = level[:, None, None] * (0.5 + rng.random((C, F, L)))
    for c in range(C):
        for b in rng.integers(0, L, peaks):
            avg[c, :, b] *= 10.0 ** rng.uniform(1.0, 4.0)
    return np.maximum(avg, 1).astype(np.float32)


def synthetic(name):
    """(config overrides, avg [C][F][L], edge [C][F] or None)"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    C, F, L = 2, 8, 256
    level = np.array([4.0, 900.0])
    cfg, edge = {}, None
    if name.startswith("scale"):
        cfg = dict(spectrum_db_scale=int(name[5:]))
        avg = spectrum(rng, C, F, L, level)
    elif name.startswith("agc"):
        cfg = dict(spectrum_agc_rate=int(name[3:]))
        avg = spectrum(rng, C, F, L, level)
    elif name.startswith("contrast"):
        cfg = dict(waterfall_contrast=int(name[8:]))
        avg = spectrum(rng, C, F, L, level)
    elif name == "scopeh16":
        cfg = dict(scope_h=16)
        avg = spectrum(rng, C, F, L, level)
    elif name == "step":
        # the level steps up and down: the AGC pulls the minimum towards 0 from both sides
        L, F = 512, 24
        cfg = dict(fft_len=L)
        steps = np.where((np.arange(F) >= 6) & (np.arange(F) < 15), 3.0e4, 1.0)
        avg = np.maximum(spectrum(rng, C, F, L, level) * steps[None, :, None], 1).astype(np.float32)
        edge = (rng.standard_normal((C, F)) * 300).astype(np.float32)
    elif name.startswith("w"):
        L, W = (int(x) for x in name[1:].split("_"))
        cfg = dict(fft_len=L, width=W)
        avg = spectrum(rng, C, F, L, level, peaks=12)
        edge = (rng.standard_normal((C, F)) * 300).astype(np.float32)
    elif name in ("edge_1e6", "edge_m1e6"):
        L = 512
        cfg = dict(fft_len=L)
        avg = spectrum(rng, C, F, L, level)
        edge = np.full((C, F), 1e6 if name == "edge_1e6" else -1e6, np.float32)
    elif name == "ones":
        avg = np.ones((C, F, L), np.float32)
    elif name == "low":
        # below 1, 0 and negative: only the stand-alone entry can see such a row
        avg = spectrum(rng, C, F, L, level)
        avg[:, :, 3::7] = (rng.random((C, F, len(range(3, L, 7)))) * 0.9).astype(np.float32)
        avg[:, :, 5::11] = 0.0
        avg[:, 1::2, 6::13] = -0.0
        avg[:, :, 8::17] = -(rng.random((C, F, len(range(8, L, 17)))) * 50).astype(np.float32)
    elif name == "nonfinite":
        avg = spectrum(rng, C, F, L, level)
        avg[0, 2:, 40] = np.nan
        avg[0, 4, 200] = np.inf
        avg[1, 1, 129] = 1e30
        avg[1, 3:, 128] = np.nan
        avg[1, 5, 0] = -np.inf
    elif name == "allnan":
        avg = np.full((C, F, L), np.nan, np.float32)
        avg[1, :3] = spectrum(rng, 1, 3, L, level[:1])[0]       # channel 1 runs three frames before the NaNs
    else:
        raise KeyError(name)
    return cfg, np.ascontiguousarray(avg, np.float32), edge


SYNTHETIC = tuple(f"scale{k}" for k in range(9)) + ("scale12", "agc1", "agc50", "contrast10", "contrast225", "scopeh16", "step",
                                                       "w512_256", "w512_300", "w512_511", "w256_200", "edge_1e6", "edge_m1e6", "ones", "low",
                                                       "nonfinite", "allnan")


def parse(raw, F, W):
    """the driver's out.bin: (scope [F][W], wfall [F][W], offset [F], min [F], edge [F], plan [3])"""
    rec = 3 * W + 12
    assert len(raw) == rec * F + 12, (len(raw), F, W)
    body = np.frombuffer(raw[:rec * F], np.uint8).reshape(F, rec)
    tail = np.ascontiguousarray(body[:, 3 * W:]).view(np.float32)
    return (np.ascontiguousarray(body[:, :2 * W]).view(np.uint16), body[:, 2 * W:3 * W].copy(), tail[:, 0].copy(), tail[:, 1].copy(),
            tail[:, 2].copy(), np.frombuffer(raw[rec * F:], np.float32).copy())


def run(driver, tmp, cfg, avg, edge):
    """one process per channel on frames of FFT_AVGData; (rows by name [C][F]..., plan [3])"""
    C, F, L = avg.shape
    r = resolved(cfg)
    W = r["width"]
    rows = dict(scope=np.empty((C, F, W), np.uint16), wfall=np.empty((C, F, W), np.uint8), offset=np.empty((C, F), np.float32),
                min=np.empty((C, F), np.float32))
    plan = None
    fin, fout = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    for c in range(C):
        with open(fin, "wb") as f:
            f.write(struct.pack("<7i", *(r[k] for k in FIELDS), F))
            for k in range(F):
                f.write(struct.pack("<f", float(edge[c, k]) if edge is not None else 0.0) + avg[c, k].tobytes())
        subprocess.run([driver, "run", fin, fout], check=True)
        scope, wfall, offset, mn, _, p = parse(open(fout, "rb").read(), F, W)
        rows["scope"][c], rows["wfall"][c], rows["offset"][c], rows["min"][c] = scope, wfall, offset, mn
        assert plan is None or plan.tobytes() == p.tobytes()
        plan = p
    return rows, plan


NYQUIST = "iq_nyquist_512"
NYQUIST_ARGS = {"mode": 0, "path": 48, "spec": 512}


def nyquist_iq():
    """I/Q with a strong component at half the sample rate, other in I than in Q: bin fft_len / 2 then has a
    real part, `edge`, large enough to move the last column of 512 -> 480, and an imaginary part that
    would move it elsewhere"""
    rng = np.random.default_rng(zlib.crc32(NYQUIST.encode()))
    C, n = 2, 2048
    sign = np.where(np.arange(n) % 2 == 0, 1, -1)[None, :]
    amp = np.array([[3.0e8, -1.5e8], [-2.0e8, 3.5e8]])          # per channel: codec word 0, codec word 1
    iq = amp[:, None, :] * sign[:, :, None] + rng.integers(-2_000_000, 2_000_000, (C, n, 2))
    return np.ascontiguousarray(iq, np.int32)


def run_spec(driver, tmp, golden, spec):
    """the harness' spectrum run of a spec_*.npz recording's I/Q (or of nyquist_iq()) with the display behind every frame"""
    if spec == NYQUIST:
        iq, args, mag, avg = nyquist_iq(), NYQUIST_ARGS, None, None
        C, F, L = iq.shape[0], iq.shape[1] // args["spec"], args["spec"]
        mag, avg = np.empty((C, F, L), np.float32), np.empty((C, F, L), np.float32)
    else:
        with np.load(os.path.join(golden, f"spec_{spec}.npz")) as z:
            iq, mag, avg, args = z["iq"], z["mag"], z["avg"], json.loads(str(z["args"]))
        C, F, L = avg.shape
    # the strong bin is the last column itself (bin fft_len / 2 lands at the row's end): a scope high enough not to clip it
    cfg = dict(DEFAULT, fft_len=L, scope_h=400 if spec == NYQUIST else 0)
    r = resolved(cfg)
    W = r["width"]
    rows = dict(scope=np.empty((C, F, W), np.uint16), wfall=np.empty((C, F, W), np.uint8), offset=np.empty((C, F), np.float32),
                min=np.empty((C, F), np.float32))
    edge = np.empty((C, F), np.float32)
    plan = None
    fin, fout, fm, fa = (os.path.join(tmp, x) for x in ("iq.bin", "out.bin", "m.bin", "a.bin"))
    for c in range(C):
        iq[c].astype(np.int32).tofile(fin)
        n = iq.shape[1]
        subprocess.run([driver, "spec", fout, *(str(r[k]) for k in FIELDS), f"in={fin}", f"n={n}", f"out_mag={fm}", f"out_avg={fa}",
                        *(f"{k}={v}" for k, v in args.items())], check=True)
        got_mag = np.fromfile(fm, np.float32)[:F * L].reshape(F, L)
        got_avg = np.fromfile(fa, np.float32)[:F * L].reshape(F, L)
        if spec == NYQUIST:
            mag[c], avg[c] = got_mag, got_avg
        assert got_mag.tobytes() == mag[c].tobytes() and got_avg.tobytes() == avg[c].tobytes(), (spec, c, "the run is not the recording's")
        scope, wfall, offset, mn, e, p = parse(open(fout, "rb").read(), F, W)
        rows["scope"][c], rows["wfall"][c], rows["offset"][c], rows["min"][c], edge[c] = scope, wfall, offset, mn, e
        assert plan is None or plan.tobytes() == p.tobytes()
        plan = p
    return cfg, iq, avg, edge, rows, plan


def reads_edge(driver, tmp, cfg):
    """whether the walk reads sd.FFT_Samples[fft_len]: a frame of ones with 0 and with an infinity there.  An
    infinity, since the float's weight can be exactly 0 (512 -> 256: samples[idx] - 1 * samples[idx]), which only
    a value that does not cancel shows"""
    probe = dict(cfg, scope_h=64, spectrum_db_scale=3)
    ones = np.ones((1, 1, cfg["fft_len"]), np.float32)
    a, _ = run(driver, tmp, probe, ones, np.zeros((1, 1), np.float32))
    b, _ = run(driver, tmp, probe, ones, np.full((1, 1), np.inf, np.float32))
    assert (a["scope"][..., :-1] == b["scope"][..., :-1]).all(), cfg
    return bool(a["scope"][0, 0, -1] != b["scope"][0, 0, -1])


def main():
    a = recording.parse_args()
    out = recording.build(a, ["display"], ["display_driver"])
    writer = recording.Recorder(a)
    driver = os.path.join(out, "display_driver")
    heights, colours, ups, downs = set(), set(), 0, 0

    with tempfile.TemporaryDirectory() as tmp:
        tab = os.path.join(tmp, "tables.bin")
        subprocess.run([driver, "tables", tab], check=True)
        raw = open(tab, "rb").read()
        num = struct.unpack("<i", raw[:4])[0]
        print("tables", writer.save("display_tables.npz", scope_scaling_factors=np.frombuffer(raw[4:], np.float32).copy(),
                                    scope_scale_num=np.int32(num)))

        for name in SPECS + (NYQUIST,) + SYNTHETIC:
            extra = {}
            if name in SPECS:
                cfg, _, avg, edge, rows, plan = run_spec(driver, tmp, a.golden, name)
                source = dict(spec=name)
            elif name == NYQUIST:
                cfg, iq, avg, edge, rows, plan = run_spec(driver, tmp, a.golden, name)
                source = dict(iq=True, args=NYQUIST_ARGS)
                extra = dict(iq=iq)
                # the recorded edge is what the last column shows: without it the column is another
                plain, _ = run(driver, tmp, cfg, avg, None)
                assert (np.abs(edge) > 1e5).all() and (rows["scope"][:, :, -1] != plain["scope"][:, :, -1]).all(), name
                again, _ = run(driver, tmp, cfg, avg, edge)
                assert all(again[k].tobytes() == rows[k].tobytes() for k in OUTPUTS), name
            else:
                over, avg, edge = synthetic(name)
                cfg = dict(DEFAULT, **over)
                rows, plan = run(driver, tmp, cfg, avg, edge)
                source = {}
            C, F, L = avg.shape
            r = resolved(cfg)
            assert L == cfg["fft_len"] and 2 <= C <= 4 and F <= 24, name
            edge_read = reads_edge(driver, tmp, cfg) if r["width"] != L else False
            if r["width"] == 480:
                assert edge_read, name
            if name == "w256_200":
                assert not edge_read, name
            if name in ("edge_1e6", "edge_m1e6"):
                # the last column shows it, and no other does
                plain, _ = run(driver, tmp, cfg, avg, None)
                assert (rows["scope"][:, :, -1] != plain["scope"][:, :, -1]).all() and (rows["wfall"][:, :, -1] != plain["wfall"][:, :, -1]).all(), name
                assert all((rows[k][:, :, :-1] == plain[k][:, :, :-1]).all() for k in ("scope", "wfall")), name
            if name == "scopeh16":
                assert rows["scope"].max() == 15 and (rows["scope"] == 15).sum() > 10, name
            if name == "allnan":
                assert (rows["min"][0] == 100000).all() and (rows["wfall"][0] == 0).all() and (rows["scope"][0] == r["scope_h"] - 1).all(), name
            if name == "scale0":
                assert (rows["min"][:, 1:] == rows["offset"][:, :-1]).all(), name        # factor 0: every sig is the offset
            if name == "edge_m1e6":
                # a negative last column: its conversion is undefined in C; what this build gives is recorded
                assert (rows["scope"][:, :, :-1] < r["scope_h"]).all() and (rows["wfall"][:, :, :-1] <= 63).all(), name
            else:
                heights |= set(rows["scope"].ravel().tolist())
                colours |= set(rows["wfall"].ravel().tolist())
            with np.errstate(invalid="ignore"):
                d = np.diff(rows["offset"], axis=1)
            ups += int((d > 0).sum())
            downs += int((d < 0).sum())
            if name == "step":
                assert (d > 0).any() and (d < 0).any() and F >= 20, name
                assert (np.abs(rows["min"][:, 5]) < np.abs(rows["min"][:, 0])).all(), name
            print(f"{name:24s} L {L} W {r['width']} edge {int(edge_read)} heights {rows['scope'].min():5d} .. {rows['scope'].max():5d} colours "
                  f"{rows['wfall'].min():3d} .. {rows['wfall'].max():3d} offset {np.nanmin(rows['offset']):9.2f} .. {np.nanmax(rows['offset']):9.2f}",
                  writer.save(f"display_{name}.npz", config=np.array(json.dumps(cfg)), source=np.array(json.dumps(source)),
                              avg=np.zeros(0, np.float32) if name in SPECS else avg, crc32=np.uint32(zlib.crc32(avg.tobytes())),
                              edge=edge if edge is not None else np.zeros((C, F), np.float32), plan=plan,
                              reads_edge=np.int32(edge_read), **extra, **rows))
    assert len(heights) > 20, sorted(heights)
    assert max(colours) == 63, sorted(colours)
    assert ups > 0 and downs > 0, (ups, downs)
    writer.finish()


if __name__ == "__main__":
    main()
