#!/usr/bin/env python3
"""Record the signal-meter fixtures (tests/golden/meter_*.npz) from the reference firmware.

Builds tools/meter/meter_driver.c with meter_spectrum_tu.c against the reference objects (meter.mk,
through oracle/ref/Makefile), runs one process per case and channel (the firmware's averages and
freq_old are statics) and records per case:

  meter_<case>.npz   the configuration, where the frames of sd.FFT_MagData come from (a spectrum
                     recording tests/golden/spec_*.npz, its frames repeated to `frames`, or the
                     frames themselves for a synthetic case) with their crc32, the cw_signal bytes,
                     Lbin / Ubin / posbin as UiSpectrum_CalculateDBm computed them, and per channel
                     and frame sm.dbm_cur, sm.dbmhz_cur, sm.dbm, sm.dbmhz, sm.s_count and
                     ads.snap_carrier_freq
  meter_tables.npz   S_Meter_Cal_dbm, and per filter path FilterInfo[id].width and the path's offset

and asserts what the set must show (tests/meter_cases.py asserts it again on load).  A recording that
has not changed leaves its file alone; --check fails where one would change.

  python3 tools/meter/make_meter_golden.py [--out DIR] [--ref DIR] [--check]
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

USB, LSB, CW, AM, SAM, FM, DIGI, SSBSTEREO, IQ = 0, 1, 2, 3, 4, 5, 6, 7, 8
SAM_BOTH, SAM_LSB, SAM_USB, SAM_STEREO = 0, 1, 2, 3
BPSK = 2
FIELDS = ("fft_len", "magnify", "iq_freq_mode", "dmod_mode", "filter_path", "sam_sideband", "cw_lsb", "digi_lsb", "digital_mode",
          "cw_sidetone_freq", "dbm_constant", "attack_alpha", "decay_alpha", "snap_enable", "tune_old")
DEFAULT = dict(fft_len=256, magnify=0, iq_freq_mode=4, dmod_mode=USB, filter_path=48, sam_sideband=SAM_BOTH, cw_lsb=0, digi_lsb=0,
               digital_mode=0, cw_sidetone_freq=750, dbm_constant=0, attack_alpha=50, decay_alpha=5, snap_enable=1, tune_old=7100000)
SNAP_MODES = "never", "always", "cw"
SPECS = ("p48_usb_256", "p48_usb_512", "p48_iqauto_256", "p48_zoom2_256", "p48_zoom16_256_p12k", "p48_zoom32_256_m6k")
SPEC_FRAMES = 8                 # a spectrum recording with fewer frames is repeated up to this many


def sample_index(L, j):
    """the bin of sd.FFT_MagData that sd.FFT_Samples[j] is taken from"""
    return (L - 1 - j + L // 2) % L


def floor(rng, C, F, L, level):
    return (level * (0.5 + rng.random((C, F, L)))).astype(np.float32)


def synthetic(name):
    """(config overrides, mag [C][F][L], cw_signal or None, tone): a noise floor and, at `tone` = the
    FFT_Samples index or None, a carrier with its two neighbours; per case below"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    C, F, L = 2, 10, 256
    cfg, cw, at = {}, None, None
    level = np.array([3.0, 40.0], np.float32)[:, None, None]       # two channels, two strengths
    amp = np.array([2.0e3, 6.0e5], np.float32)[:, None]

    def carrier(mag, j, skew=0.3):
        mag[:, :, sample_index(L, j)] = amp * (1 + 0.02 * np.arange(F, dtype=np.float32))
        if 0 < j:
            mag[:, :, sample_index(L, j - 1)] = amp * skew
        if j < L - 1:
            mag[:, :, sample_index(L, j + 1)] = amp * skew * 0.5
        return mag

    if name.startswith("cw300"):
        cfg = dict(dmod_mode=CW, filter_path=4 if "p4" in name else 9, cw_lsb=int(name.endswith("lsb")))
        cw = np.tile(np.array([0, 0, 1, 1, 0, 1, 0, 0, 1, 1], np.uint8), (C, 1))
        cw[1] = 1 - cw[1]
        mag = floor(rng, C, F, L, 1.0) * level
        mag[:, :, :] += (amp[:, :, None] * rng.random((C, F, L)) * 0.01).astype(np.float32)     # the maximum moves from frame to frame
    elif name == "cw_onebin":
        # 300 Hz centred on 900 Hz, lower sideband, magnify 5: bw_UPPER = -750 Hz is exactly -128 bins of 5.859375 Hz, so
        # Ubin = 0, and Lbin, negative, is clamped to 0: a passband of one bin, where the dBm/Hz term is 10 log10(0)
        cfg = dict(dmod_mode=CW, filter_path=12, cw_lsb=1, magnify=5)
        cw = np.tile(np.array([0, 1, 1, 0, 1, 0, 0, 1, 1, 0], np.uint8), (C, 1))
        cw[1] = 1 - cw[1]
        mag = floor(rng, C, F, L, 1.0) * level
        mag += (amp[:, :, None] * rng.random((C, F, L)) * 0.01).astype(np.float32)
    elif name in ("am", "sam_both", "sam_lsb", "sam_usb", "sam_stereo", "fm", "ssbstereo", "iq"):
        # fm, ssbstereo, iq and sam_stereo: the other modes RadioManagement_UsesBothSidebands names (two-channel audio)
        cfg = dict(dmod_mode={"am": AM, "fm": FM, "ssbstereo": SSBSTEREO, "iq": IQ}.get(name, SAM), filter_path=2,
                   sam_sideband={"sam_lsb": SAM_LSB, "sam_usb": SAM_USB, "sam_stereo": SAM_STEREO}.get(name, SAM_BOTH))
        mag = floor(rng, C, F, L, 1.0) * level
        mag += (amp[:, :, None] * rng.random((C, F, L)) * 0.01).astype(np.float32)
    elif name.startswith("bpsk"):
        cfg = dict(dmod_mode=DIGI, digital_mode=BPSK, digi_lsb=int(name.endswith("lsb")))
        mag = floor(rng, C, F, L, 1.0) * level
        mag += (amp[:, :, None] * rng.random((C, F, L)) * 0.01).astype(np.float32)
    elif name.startswith("iqmode"):
        cfg = dict(iq_freq_mode=int(name[-1]))
        mag = floor(rng, C, F, L, 1.0) * level * 100
    elif name.startswith("dbmc"):
        cfg = dict(dbm_constant=100 if name.endswith("p100") else -100)
        mag = floor(rng, C, F, L, 1.0) * level * 100
    elif name.startswith("alpha"):
        a = int(name.split("_")[1])
        cfg = dict(attack_alpha=a, decay_alpha=a)
        F = 12
        mag = floor(rng, C, F, L, 1.0) * level * np.where(np.arange(F) % 6 < 3, 1.0, 300.0).astype(np.float32)[None, :, None]
    elif name == "step":
        F = 24
        steps = np.where((np.arange(F) >= 6) & (np.arange(F) < 14), 3.0e4, 1.0).astype(np.float32)
        mag = floor(rng, C, F, L, 1.0) * level * steps[None, :, None]
    elif name == "tone_bin0":
        cfg, at = dict(dmod_mode=AM, filter_path=2, magnify=5), 0
        mag = carrier(floor(rng, C, F, L, 1.0) * level, at)
    elif name == "tone_lbin":
        cfg, at = dict(dmod_mode=AM, filter_path=2), "lbin"
        mag = floor(rng, C, F, L, 1.0) * level
    elif name == "zero":
        cfg = dict(dmod_mode=AM, filter_path=2)
        mag = np.zeros((C, F, L), np.float32)
    elif name == "denormal":
        cfg = dict(dmod_mode=AM, filter_path=2)
        mag = (np.float32(1e-42) * (1 + rng.integers(0, 50, (C, F, L)))).astype(np.float32)
    elif name in ("nan", "inf"):
        cfg, at = dict(dmod_mode=AM, filter_path=2), 190
        mag = carrier(floor(rng, C, F, L, 1.0) * level, at)
        bad = np.float32(np.nan) if name == "nan" else np.float32(np.inf)
        mag[0, 3:, sample_index(L, at + 9)] = bad       # channel 0: apart from the carrier, from frame 3 on
        mag[1, 5, sample_index(L, at + 1)] = bad        # channel 1: beside it, in one frame
    elif name == "huge_1e30":
        cfg = dict(dmod_mode=AM, filter_path=2)
        mag = np.full((C, F, L), 1e30, np.float32)
    elif name == "overflow":
        cfg = dict(dmod_mode=AM, filter_path=2)
        mag = np.full((C, F, L), 3e35, np.float32)
        mag[1] = np.float32(2e34)                       # channel 1: the three samples still add up, the passband does not
    else:
        raise KeyError(name)
    return cfg, np.ascontiguousarray(mag, np.float32), cw, at


SYNTHETIC = ("cw300_p4_usb", "cw300_p9_lsb", "cw_onebin", "sam_stereo", "fm", "ssbstereo", "iq", "am", "sam_both", "sam_lsb", "sam_usb", "bpsk_usb", "bpsk_lsb", "iqmode0", "iqmode1",
             "iqmode2", "iqmode3", "dbmc_p100", "dbmc_m100", "alpha_1_1", "alpha_100_100", "step", "tone_bin0", "tone_lbin", "zero",
             "denormal", "nan", "inf", "huge_1e30", "overflow")


def spec_case(golden, spec, lsb):
    with np.load(os.path.join(golden, f"spec_{spec}.npz")) as z:
        mag, args = z["mag"], json.loads(str(z["args"]))
    frames = max(SPEC_FRAMES, mag.shape[1])
    cfg = dict(fft_len=args["spec"], magnify=args.get("mag", 0), iq_freq_mode=args.get("iqmode", 4), dmod_mode=LSB if lsb else USB)
    return cfg, spec_frames(mag, frames), dict(spec=spec, frames=frames)


def spec_frames(mag, frames):
    return np.ascontiguousarray(mag[:, np.arange(frames) % mag.shape[1]])


def run(driver, tmp, cfg, mag, cw):
    """one process per channel; (six rows [C][F], bins [3])"""
    C, F, L = mag.shape
    rows = [np.empty((C, F), dt) for dt in (np.float32,) * 4 + (np.int32, np.uint32)]
    bins = None
    fin, fout = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    for c in range(C):
        head = [2 * cfg["fft_len"], cfg["magnify"], cfg["iq_freq_mode"], cfg["dmod_mode"], cfg["filter_path"], cfg["sam_sideband"],
                cfg["cw_lsb"], cfg["digi_lsb"], int(cfg["digital_mode"] == BPSK), cfg["cw_sidetone_freq"], cfg["dbm_constant"],
                cfg["attack_alpha"], cfg["decay_alpha"], cfg["snap_enable"], cfg["tune_old"], F]
        with open(fin, "wb") as f:
            f.write(struct.pack("<16i", *head))
            for k in range(F):
                f.write(struct.pack("<i", int(cw[c, k]) if cw is not None else 0) + mag[c, k].tobytes())
        subprocess.run([driver, "run", fin, fout], check=True)
        raw = open(fout, "rb").read()
        assert len(raw) == 24 * F + 12, (len(raw), F)
        rec = np.frombuffer(raw[:24 * F], np.uint32).reshape(F, 6)
        for k, r in enumerate(rows):
            r[c] = rec[:, k].view(r.dtype)
        b = np.frombuffer(raw[24 * F:], np.int32)
        assert bins is None or np.array_equal(bins, b)
        bins = b.copy()
    return rows, bins


def first_maximum(mag, L, lbin, ubin):
    """maxbin of UiSpectrum_CalculateSnap per frame of mag [F][L]"""
    s = mag[:, [sample_index(L, j) for j in range(lbin, ubin + 1)]] * np.float32(1000)
    s = np.where(s > 0, s, 0)           # a NaN or nothing above zero never wins
    return np.where(s.max(axis=1) > 0, lbin + s.argmax(axis=1), 1)


def main():
    a = recording.parse_args()
    out = recording.build(a, ["meter"], ["meter_driver"])
    writer = recording.Recorder(a)
    driver = os.path.join(out, "meter_driver")
    names = ("dbm_cur", "dbmhz_cur", "dbm", "dbmhz", "s_count", "snap_carrier_freq")
    s_counts, rises, falls = set(), 0, 0

    with tempfile.TemporaryDirectory() as tmp:
        tab = os.path.join(tmp, "tables.bin")
        subprocess.run([driver, "tables", tab], check=True)
        raw = open(tab, "rb").read()
        widths = np.frombuffer(raw[132:], np.uint16).reshape(-1, 2)
        print("tables", writer.save("meter_tables.npz", s_meter_cal_dbm=np.frombuffer(raw[:132], np.float32).copy(),
                                    path_width=widths[:, 0].copy(), path_offset=widths[:, 1].copy()))

        cases = [(f"{spec}_{'lsb' if lsb else 'usb'}", spec, lsb) for spec in SPECS for lsb in (0, 1)] + [(n, None, 0) for n in SYNTHETIC]
        for name, spec, lsb in cases:
            if spec:
                over, mag, source = spec_case(a.golden, spec, lsb)
                cw, at = None, None
            else:
                over, mag, cw, at = synthetic(name)
                source = {}
            cfg = dict(DEFAULT, **over)
            C, F, L = mag.shape
            assert L == cfg["fft_len"] and F >= 8, name
            if at == "lbin":
                # the carrier at Lbin itself: one probe run tells where that is
                _, bins = run(driver, tmp, cfg, mag[:1, :1], None)
                amp = np.array([2.0e3, 6.0e5], np.float32)[:, None]
                mag[:, :, sample_index(L, int(bins[0]))] = amp * (1 + 0.02 * np.arange(F, dtype=np.float32))
                mag[:, :, sample_index(L, int(bins[0]) - 1)] = amp * 2        # outside the passband, larger: must not win
                mag[:, :, sample_index(L, int(bins[0]) + 1)] = amp * 0.4
            rows, bins = run(driver, tmp, cfg, mag, cw)
            lbin, ubin, posbin = (int(x) for x in bins)
            assert 0 <= lbin <= ubin <= L - 1, (name, bins)
            dmod = cfg["dmod_mode"]
            carrier = dmod in (AM, SAM) or (dmod == DIGI and cfg["digital_mode"] == BPSK)
            snap_mode = 0 if not cfg["snap_enable"] else 1 if carrier else 2 if dmod == CW else 0
            snap = rows[5]
            for c in range(C):
                runs = np.ones(F, bool) if snap_mode == 1 else (cw[c] != 0) if snap_mode == 2 else np.zeros(F, bool)
                prev = np.concatenate([[0], snap[c, :-1]])
                assert (snap[c][~runs] == prev[~runs]).all(), (name, "snap_carrier_freq moved on a frame without SNAP")
                if runs.any():
                    assert (snap[c][runs] != prev[runs]).any(), (name, "snap_carrier_freq never moved")
                    mb = first_maximum(mag[c][runs], L, lbin, ubin)
                    assert (mb != L - 1).all(), (name, "maxbin == L - 1: choose other input")
                    if at == 0:
                        assert (mb == 0).all(), name
                    if at == "lbin":
                        assert (mb == lbin).all(), name
            s_counts |= set(int(x) for x in rows[4].ravel())
            with np.errstate(invalid="ignore"):
                d = np.diff(rows[2], axis=1)        # inf - inf in the overflow cases
            rises += int((d > 0).sum())
            falls += int((d < 0).sum())
            if name == "cw_onebin":
                assert [lbin, ubin, posbin] == [0, 0, 128] and np.isfinite(rows[1]).all(), (name, bins)
            if name in ("sam_stereo", "fm", "ssbstereo", "iq"):
                assert posbin - lbin == ubin - posbin > 0 and snap_mode == (name == "sam_stereo"), (name, bins)
            if name == "zero":
                assert (rows[0] == -145).all() and (rows[1] == -145).all(), name
            print(f"{name:28s} L {L} bins [{lbin:3d}, {ubin:3d}] posbin {posbin:3d} snap {SNAP_MODES[snap_mode]:6s} dbm {np.nanmin(rows[2]):9.2f} .. "
                  f"{np.nanmax(rows[2]):9.2f}  s_count {sorted(set(rows[4].ravel().tolist()))}  {snap[0, -1]}",
                  writer.save(f"meter_{name}.npz", config=np.array(json.dumps(cfg)), source=np.array(json.dumps(source)),
                              mag=np.zeros(0, np.float32) if spec else mag, crc32=np.uint32(zlib.crc32(mag.tobytes())),
                              cw_signal=cw if cw is not None else np.zeros((C, F), np.uint8), bins=bins.astype(np.int32),
                              **dict(zip(names, rows))))
    assert len(s_counts) >= 5, s_counts
    assert rises > 0 and falls > 0, (rises, falls)      # both branches of the averager pair
    writer.finish()


if __name__ == "__main__":
    main()
