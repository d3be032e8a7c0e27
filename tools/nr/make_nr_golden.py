#!/usr/bin/env python3
"""Record the noise-reduction fixtures (tests/golden/nr_*.npz) from the reference firmware.

Builds tools/nr/nr_driver.c and tools/nr/nr_stream.c against the reference objects (nr.mk, through
oracle/ref/Makefile), generates each case's input with uhsdr_amd.synth.nr_audio, runs one process
per case and records:

  nr_tables.npz          SQRT_von_Hann_256, NR_decimate_coeffs, NR_interpolate_coeffs as the compiled
                         reference holds them (tools/nr/gen_nr_tables.py writes the library's header)
  nr_icfft.npz           256-point inputs and arm_cfft_f32(.., 1, 1) of them
  nr_<case>.npz          frame cases: the generator's arguments, a crc32 of the input, the
                         configuration, per frame NN, power_ratio and first_time, and the complete
                         output (short cases) or a crc32 per frame plus the first and last 8 frames
  nr_stream_<case>.npz   stream cases (AudioDriver_RxProcessorNoiseReduction in blocks of 8 with
                         AudioNr_HandleNoiseReduction after each): the complete output

and asserts what each case is there to show.  A recording that has not changed leaves its file alone;
--check fails where one would change.

  python3 tools/nr/make_nr_golden.py [--out DIR] [--ref DIR] [--check]
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
ALPHA_DEFAULT = 0.94                       # NR_Init
SHORT = 64                                 # frames up to which the whole output is kept


def alpha_from_strength(s):
    """audio_driver.c:1195, 0.799 + ((float32_t)nr_strength / 1000.0) assigned to a float"""
    return float(np.float32(0.799 + float(np.float32(s)) / 1000.0))


def config(alpha=ALPHA_DEFAULT, asnr=30, width=4, power_threshold_int=40, width_hz=2700, offset_hz=1650, sample_rate=6000):
    return dict(alpha=float(np.float32(alpha)), asnr=asnr, width=width, power_threshold_int=power_threshold_int,
                width_hz=width_hz, offset_hz=offset_hz, sample_rate=sample_rate)


def frame_cases():
    """name, frames, generator arguments, configuration, frame at which the run restarts, what to show"""
    def case(name, frames, cfg, reset=-1, show=None, **gen):
        g = dict(nsamples=frames * FRAME, rate=float(cfg["sample_rate"]), snr_db=10.0, seed=len(name))
        g.update(gen)
        return dict(name=name, frames=frames, cfg=cfg, reset=reset, show=show, gen=g)
    ssb = dict(width_hz=2700, offset_hz=1650)
    return [
        case("ssb6k_snr10", 48, config(**ssb)),
        case("ssb6k_snrm3_weak", 48, config(alpha=alpha_from_strength(1), asnr=15, **ssb), snr_db=-3.0),
        case("ssb6k_snr20_strong", 48, config(alpha=alpha_from_strength(200), asnr=30, **ssb), snr_db=20.0),
        case("ssb6k_snr3_asnr15", 48, config(asnr=15, **ssb), snr_db=3.0),
        case("cw6k_snr5", 48, config(width_hz=200, offset_hz=400), snr_db=5.0),
        case("wide12k_snr10", 48, config(width_hz=2900, offset_hz=1550, sample_rate=12000)),
        case("wide12k_snrm3", 48, config(width_hz=3600, offset_hz=1900, sample_rate=12000, alpha=alpha_from_strength(1)), snr_db=-3.0),
        case("equal_band", 48, config(width_hz=10, offset_hz=500), show="equal", snr_db=5.0),
        case("wrap126", 48, config(width_hz=2700, offset_hz=1000), show="wrap"),
        case("restart", 60, config(**ssb), reset=33, snr_db=5.0),
        case("nn_all", 400, config(**ssb), show="nn_all", snr_db=0.0),
        case("width5_thr100", 48, config(width=5, power_threshold_int=100, **ssb), show="nn11", snr_db=0.0),
    ]


def stream_cases():
    def case(name, nsamples, cfg, **gen):
        g = dict(nsamples=nsamples, rate=12000.0, snr_db=8.0, seed=100 + len(name))
        g.update(gen)
        return dict(name=name, cfg=cfg, gen=g)
    return [
        case("ssb", 8000, config(width_hz=2700, offset_hz=1650)),
        case("cw", 8000, config(width_hz=200, offset_hz=400, alpha=alpha_from_strength(1), asnr=15), snr_db=3.0),
        case("wide", 8000, config(width_hz=2900, offset_hz=1550, sample_rate=12000)),
    ]


def alpha_bits(cfg):
    return str(struct.unpack("<I", struct.pack("<f", cfg["alpha"]))[0])


def band(cfg):
    """VAD_low, VAD_high before the clamps, as the C computes them in binary32"""
    f = np.float32
    bw = f(cfg["sample_rate"]) / f(256)
    lf = (f(cfg["offset_hz"]) - f(cfg["width_hz"]) / f(2)) / bw
    uf = (f(cfg["offset_hz"]) + f(cfg["width_hz"]) / f(2)) / bw
    return int(lf) & 255, int(uf) & 255


def main():
    a = recording.parse_args()
    out = recording.build(a, ["nr"], ["nr_driver", "nr_stream"])
    writer = recording.Recorder(a)
    drv, strm = os.path.join(out, "nr_driver"), os.path.join(out, "nr_stream")

    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.bin")

        subprocess.run([drv, "tables", fout], check=True)
        window = np.fromfile(fout, dtype=np.float32)
        subprocess.run([strm, "tables", fout], check=True)
        fir = np.fromfile(fout, dtype=np.float32)
        assert len(window) == 256 and len(fir) == 44
        writer.save("nr_tables.npz", sqrt_hann_256=window, decimate=fir[:4].copy(), interpolate=fir[4:].copy())

        # inverse transform vectors: an impulse, a spectrum with conjugate symmetry, random complex
        # values without it, one bin alone, and values spread over 60 decades with a negative zero
        rng = np.random.default_rng(20261020)
        x = np.zeros((5, 256), np.complex64)
        x[0, 3] = 1.0
        half = (rng.standard_normal(127) + 1j * rng.standard_normal(127)).astype(np.complex64)
        x[1, 1:128], x[1, 129:] = half, np.conj(half[::-1])
        x[1, 0], x[1, 128] = 5.0, -2.0
        x[2] = (rng.standard_normal(256) + 1j * rng.standard_normal(256)).astype(np.complex64) * 1000
        x[3, 37] = 256.0 - 128.0j
        x[4] = ((rng.standard_normal(256) + 1j * rng.standard_normal(256)) * 10.0 ** rng.integers(-30, 30, 256)).astype(np.complex64)
        x[4, 0] = complex(-0.0, 0.0)
        xin = np.ascontiguousarray(x).view(np.float32).reshape(5, 512)
        xin.tofile(fin)
        subprocess.run([drv, "icfft", fin, fout], check=True)
        writer.save("nr_icfft.npz", x=xin.copy(), y=np.fromfile(fout, dtype=np.float32).reshape(5, 512))

        for c in frame_cases():
            audio = synth.nr_audio(**c["gen"])
            audio.tofile(fin)
            cfg = c["cfg"]
            args = [drv, "frames", fin, fout, alpha_bits(cfg)] + [str(cfg[k]) for k in
                                                                   ("asnr", "width", "power_threshold_int", "width_hz", "offset_hz", "sample_rate")]
            if c["reset"] >= 0:
                args.append(str(c["reset"]))
            subprocess.run(args, check=True)
            r = np.fromfile(fout, dtype=np.uint32).reshape(-1, 259)
            assert len(r) == c["frames"]
            y = r[:, :128].copy().view(np.float32)
            hk_last = r[-1, 128:256].copy().view(np.float32)
            nn, ratio, first_time = r[:, 256].astype(np.int32), r[:, 257].copy().view(np.float32), r[:, 258].astype(np.int32)
            seen = sorted(set(nn[19:].tolist()))       # NN is a frame's own only once the noise reduction runs
            lo, hi = band(cfg)
            print(f"{c['name']:22s} {c['frames']:4d} frames  band {lo:3d} {hi:3d}  NN {seen}")
            assert np.isfinite(y).all(), c["name"]
            assert first_time[18] == 2 and first_time[19] == 3, c["name"]
            if c["show"] == "nn_all":
                assert seen == [1, 3, 5, 7, 9], f"{c['name']}: NN takes {seen}"
            elif c["show"] == "nn11":
                assert 11 in seen, f"{c['name']}: NN takes {seen}"
            elif c["show"] == "equal":
                assert lo == hi, f"{c['name']}: band {lo} {hi}"
            elif c["show"] == "wrap":
                # nothing is weighted: the output is the input one frame later under the window's
                # overlap-add, w[i]^2 + w[i + 128]^2, which is within 0.62 % of 1 for this table
                delayed = audio.reshape(-1, FRAME)[:-1].astype(np.float64)
                gain = window[:128].astype(np.float64) ** 2 + window[128:].astype(np.float64) ** 2
                assert abs(gain - 1).max() < 0.0062
                assert lo > 126 and np.abs(y[1:] - delayed * gain).max() <= 1e-5 * np.abs(delayed).max(), c["name"]
                assert np.isnan(ratio[19:]).all() and seen == [1], c["name"]
            if c["reset"] >= 0:
                assert first_time[c["reset"] - 1] == 3 and first_time[c["reset"]] == 2, c["name"]
            arrays = dict(gen=np.array(json.dumps(c["gen"])), config=np.array(json.dumps(cfg)), samples=np.int32(len(audio)),
                          crc32=np.uint32(zlib.crc32(audio.tobytes())), reset=np.int32(c["reset"]), nn=nn, power_ratio=ratio,
                          first_time=first_time, hk_last=hk_last)
            if c["frames"] <= SHORT:
                arrays["out"] = y
            else:
                arrays["out_crc"] = np.array([zlib.crc32(f.tobytes()) for f in y], dtype=np.uint32)
                arrays["out_head"], arrays["out_tail"] = y[:8].copy(), y[-8:].copy()
            writer.save(f"nr_{c['name']}.npz", **arrays)

        for c in stream_cases():
            audio = synth.nr_audio(**c["gen"])
            audio.tofile(fin)
            cfg = c["cfg"]
            subprocess.run([strm, "run", fin, fout, alpha_bits(cfg)] + [str(cfg[k]) for k in
                           ("asnr", "width", "power_threshold_int", "width_hz", "offset_hz")], check=True)
            y = np.fromfile(fout, dtype=np.float32)
            assert len(y) == len(audio) and np.isfinite(y).all(), c["name"]
            # the latency the recording shows: two frames at the frames' rate, silence until then
            first = int(np.argmax(y != 0))
            decimated = cfg["width_hz"] < 2701
            print(f"stream_{c['name']:15s} {len(audio):6d} samples  first output at {first}")
            assert (first >= 512 and first < 540) if decimated else first == 257, c["name"]
            writer.save(f"nr_stream_{c['name']}.npz", gen=np.array(json.dumps(c["gen"])),
                        config=np.array(json.dumps(cfg)), samples=np.int32(len(audio)), crc32=np.uint32(zlib.crc32(audio.tobytes())), out=y)
    writer.finish()


if __name__ == "__main__":
    main()
