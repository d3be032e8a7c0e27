#!/usr/bin/env python3
"""Throughput of the spectral noise reduction on voiced / keyed signals in noise
(uhsdr_amd.synth.nr_audio, 64 different rows tiled over the channels): the frame stage alone
(uhsdr_nr_process_frames, kernel nr_frames, --frames frames of 128 samples a call at 6 ksps) and
the 12 ksps stream around it (uhsdr_nr_process: decimator, frames, FIFO, interpolator; the same
number of frames a call, so 256 * frames input samples).

    python tools/bench_nr.py [--channels 65536] [--frames 16] [--calls 50] [--runs 3] [--out FILE]
    python tools/bench_nr.py --samples 64 --width-hz 3800 --offset-hz 1900 [--nb-setting 8] --channels 131072
        the stream alone at a call of --samples 12 ksps samples (a multiple of 8, the RX chain's N / 4) and that
        filter width: the yardstick of the stage inside the RX chain (bench_configs.py --only c5nr)

Prints one JSON line per run and level: ms per call and frames per second, timed with device events
over the calls after a warm-up of 24 calls (past the 20-frame start-up, so the timed calls run the
noise reduction proper); --out appends the lines to a file."""
import argparse

import numpy as np

from benchlib import emit, rows_on_device, timed

WARMUP = 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--samples", type=int, default=0, help="time the stream alone at this many 12 ksps samples a call")
    ap.add_argument("--width-hz", type=int, default=2700)
    ap.add_argument("--offset-hz", type=int, default=1650)
    ap.add_argument("--nb-setting", type=int, default=0)
    a = ap.parse_args()
    import torch
    from uhsdr_amd import nr, synth
    C, F = a.channels, a.frames
    s = torch.cuda.current_stream()
    if a.samples:
        n = a.samples
        warm = (WARMUP * nr.FRAME * (2 if a.width_hz < 2701 else 1) + n - 1) // n      # past the 20-frame start-up
        base = np.stack([synth.nr_audio(n, rate=12000.0, snr_db=-3.0 + 0.36 * k, seed=k) for k in range(64)])
        x = rows_on_device(torch, base, C)
        y = torch.empty_like(x)
        for run in range(a.runs):
            p = nr.NrProcessor(C, nr.nr_config(width_hz=a.width_hz, offset_hz=a.offset_hz, nb_setting=a.nb_setting), stream=s.cuda_stream)
            ms = timed(torch, lambda: p.process(x, y), a.calls, warm)
            ft = p.state()[0]
            p.close()
            emit({"workload": f"nr stream: {n} samples at 12 ksps a call, width {a.width_hz} Hz, nb_setting {a.nb_setting}",
                  "level": "stream", "channels": C, "samples_per_call": n, "calls": a.calls, "warmup_calls": warm, "run": run,
                  "ms_per_call": round(ms, 4), "first_time": sorted(set(ft.tolist()))}, a.out)
        return
    for level, n, rate in (("frames", F * nr.FRAME, 6000.0), ("stream", 2 * F * nr.FRAME, 12000.0)):
        base = np.stack([synth.nr_audio(n, rate=rate, snr_db=-3.0 + 0.36 * k, seed=k) for k in range(64)])
        x = rows_on_device(torch, base, C)
        y = torch.empty_like(x)
        for run in range(a.runs):
            p = nr.NrProcessor(C, nr.nr_config(), stream=s.cuda_stream)
            call = (lambda: p.process_frames(x, y)) if level == "frames" else (lambda: p.process(x, y))
            ms = timed(torch, call, a.calls, WARMUP)
            nn = p.state()[1]
            p.close()
            emit({"workload": f"nr {level}: {F} frames of 128 samples a call at 6 ksps, signals in noise tiled over the channels",
                  "level": level, "channels": C, "frames_per_call": F, "calls": a.calls, "warmup_calls": WARMUP, "run": run,
                  "ms_per_call": round(ms, 4), "frames_per_s": round(C * F / (ms * 1e-3), 0),
                  "ns_per_channel_frame": round(ms * 1e6 / (C * F), 3),
                  "realtime_channels_at_6ksps": round(C * F / (ms * 1e-3) / (6000.0 / nr.FRAME), 0),
                  "nn_values": sorted(set(nn.tolist()))}, a.out)
        del x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
