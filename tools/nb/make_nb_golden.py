#!/usr/bin/env python3
"""Record the noise-blanker fixtures (tests/golden/nb_*.npz) from the reference firmware.

Builds tools/nb/nb_driver.c and tools/nb/nb_stream.c against the reference objects (nr.mk and nb.mk,
through oracle/ref/Makefile), generates each case's input with uhsdr_amd.synth.nb_audio, runs one
process per case and records:

  nb_<case>.npz          frame cases (AudioNr_RunNoiseReduction with the blanker alone): the
                         generator's arguments, a crc32 of the input, the setting and the complete
                         output
  nb_stream_<case>.npz   stream cases (AudioDriver_RxProcessorNoiseReduction in blocks of 8 with
                         AudioNr_HandleNoiseReduction after each, the blanker alone or in front of
                         the noise reduction): the same with the noise reduction's configuration

and asserts what each case is there to show (tests/nb_cases.py asserts it again on load).  A
recording that has not changed leaves its file alone; --check fails where one would change.

  python3 tools/nb/make_nb_golden.py [--out DIR] [--ref DIR] [--check]
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
from uhsdr_amd import synth  # noqa: E402

FRAME = 128
DELAY = 13
FRAMES = 56
N = FRAMES * FRAME

# impulses of 4 000 to 30 000 (the weak ones pass a low setting) on audio of a few thousand
SPARSE = [[900 + 701 * j, (4000.0 + 3250.0 * j) * (-1) ** j] for j in range(9)]
BURST = [[20 * FRAME + 10 + 14 * j, 25000.0 * (-1) ** j] for j in range(8)]
# one impulse per frame boundary, at -16 .. +15 samples from it
WALK = [[(10 + j) * FRAME + (j - 16), 25000.0 * (-1) ** j] for j in range(32)]


def frame_cases():
    def case(name, setting, show, **gen):
        g = dict(nsamples=N, seed=len(name))
        g.update(gen)
        return dict(name=name, setting=setting, show=show, gen=g)
    return [
        case("sparse_s1", 1, "changed", seed=1, impulses=SPARSE),
        case("sparse_s8", 8, "changed", seed=1, impulses=SPARSE),
        case("sparse_s15", 15, "changed", seed=1, impulses=SPARSE),
        case("burst8", 8, "burst", impulses=BURST),
        case("walk", 8, "walk", impulses=WALK),
        case("tone", 8, "changed", kind="tone", sigma=30.0, impulses=SPARSE),
        case("noise_s15", 15, "every", kind="noise"),
        case("clean_s8", 8, "same"),
        case("dc", 8, "same", kind="dc", ramp=512),
        case("silence", 8, "same", kind="silence"),
        case("tiny", 8, "same", scale=1e-22),
        case("big", 8, "finite", seed=1, impulses=SPARSE, scale=1e14),
        case("nan_inf", 8, "nan", seed=1, impulses=SPARSE, nan_at=3000, inf_at=5000),
    ]


def nr_config(width_hz, offset_hz):
    return dict(alpha=float(np.float32(0.94)), asnr=30, width=4, power_threshold_int=40, width_hz=width_hz, offset_hz=offset_hz,
                sample_rate=6000)


def stream_cases():
    imp = [[300 + 611 * j, (20000.0 + 1400.0 * j) * (-1) ** j] for j in range(7)]

    def case(name, setting, nr_on, width_hz, offset_hz):
        cfg = nr_config(width_hz, offset_hz)
        cfg.update(nb_setting=setting, nr_bypass=0 if nr_on else 1)
        return dict(name=name, cfg=cfg, gen=dict(nsamples=600 * 8, seed=100 + len(name), impulses=imp))
    return [
        case("nb_wide", 8, False, 3200, 1700),
        case("nb_narrow", 8, False, 2400, 1500),
        case("nb_nr_2700", 8, True, 2700, 1650),
        case("nb_nr_wide", 8, True, 3200, 1700),
    ]


def changed(x, y, delay=DELAY):
    """which output samples differ in their bits from the input `delay` samples earlier"""
    d = np.concatenate([np.zeros(delay, np.float32), x])[:len(y)]
    return d.view(np.uint32) != y.view(np.uint32)


def run_starts(mask):
    """first index of every run of set elements"""
    m = np.concatenate([[False], mask])
    return np.flatnonzero(m[1:] & ~m[:-1])


def main():
    a = recording.parse_args()
    out = recording.build(a, ["nr", "nb"], ["nb_driver", "nb_stream"])
    writer = recording.Recorder(a)
    drv, strm = os.path.join(out, "nb_driver"), os.path.join(out, "nb_stream")

    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.f32")
        counts = {}
        for c in frame_cases():
            x = synth.nb_audio(**c["gen"])
            x.tofile(fin)
            subprocess.run([drv, "frames", fin, fout, str(c["setting"])], check=True)
            y = np.fromfile(fout, dtype=np.float32)
            assert len(y) == len(x) == N, c["name"]
            ch = changed(x, y)
            per_frame = ch.reshape(-1, FRAME).sum(axis=1)
            counts[c["name"]] = int(ch.sum())
            print(f"{c['name']:12s} setting {c['setting']:2d}  changed {int(ch.sum()):5d} samples in {int((per_frame > 0).sum()):2d} frames, "
                  f"most in one frame {int(per_frame.max())}")
            show = c["show"]
            if show == "same":
                assert not ch.any(), c["name"]
            else:
                assert ch.any(), c["name"]
            if show == "burst":
                assert per_frame.max() > 28, c["name"]
            if show == "walk":
                at = (run_starts(ch) - DELAY) % FRAME
                assert (at >= 96).any() and (at < 32).any(), c["name"]
            if show == "every":
                assert (per_frame[1:] > 0).all(), c["name"]
            if show == "nan":
                assert int(np.isnan(y).sum()) == 1, c["name"]
            else:
                assert np.isfinite(y).all(), c["name"]
            writer.save(f"nb_{c['name']}.npz", gen=np.array(json.dumps(c["gen"])),
                        config=np.array(json.dumps(dict(nb_setting=c["setting"]))), samples=np.int32(len(x)),
                        crc32=np.uint32(zlib.crc32(x.tobytes())), out=y)
        assert counts["sparse_s1"] < counts["sparse_s8"] < counts["sparse_s15"], counts

        for c in stream_cases():
            x = synth.nb_audio(**c["gen"])
            x.tofile(fin)
            cfg = c["cfg"]
            bits = str(struct.unpack("<I", struct.pack("<f", cfg["alpha"]))[0])
            subprocess.run([strm, "run", fin, fout, bits] + [str(cfg[k]) for k in ("asnr", "width", "power_threshold_int", "width_hz", "offset_hz",
                                                                                    "nb_setting")] + [str(1 - cfg["nr_bypass"])], check=True)
            y = np.fromfile(fout, dtype=np.float32)
            assert len(y) == len(x) and np.isfinite(y).all(), c["name"]
            first = int(np.argmax(y != 0))
            print(f"stream_{c['name']:12s} {len(x):5d} samples  first output at {first}")
            if c["name"] == "nb_wide":
                ch = changed(x, y, 256 + DELAY)
                print(f"{'':19s} changed {int(ch.sum())} samples")
                assert not y[:256 + DELAY].any() and 0 < ch.sum() <= 7 * 5 * (len(x) // FRAME), c["name"]
            else:
                assert first >= (256 if cfg["width_hz"] >= 2701 else 512), c["name"]
            writer.save(f"nb_stream_{c['name']}.npz", gen=np.array(json.dumps(c["gen"])),
                        config=np.array(json.dumps(cfg)), samples=np.int32(len(x)), crc32=np.uint32(zlib.crc32(x.tobytes())), out=y)
    writer.finish()


if __name__ == "__main__":
    main()
