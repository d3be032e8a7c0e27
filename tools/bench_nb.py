#!/usr/bin/env python3
"""Throughput of the noise blanker on voiced audio (uhsdr_amd.synth.nb_audio, 64 different rows
tiled over the channels, every second one with impulses): the blanker's frames alone
(uhsdr_nb_process_frames, kernel nb_frames, --frames frames of 128 samples a call) and the 12 ksps
stream (uhsdr_nr_process at a filter width of 3200 Hz, the same number of frames a call) with the
noise reduction alone and with the blanker in front of it.

    python tools/bench_nb.py [--channels 4096,65536,262144] [--frames 16] [--calls 30] [--runs 3] [--out FILE]

Prints one JSON line per run, shape and level: ms per call and frames per second, timed with device
events over the calls after a warm-up of 24 calls (past the noise reduction's 20-frame start-up), and
for the blanker the share of channels (lanes) that repaired at least one place in the timed calls
and the places repaired per channel-frame: repairs are divergent work.  --out appends the lines to
a file."""
import argparse

import numpy as np

from benchlib import emit, rows_on_device, timed

WARMUP = 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="4096,65536,262144")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--setting", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from uhsdr_amd import nb, nr, synth
    F = a.frames
    n = F * nb.FRAME
    s = torch.cuda.current_stream()
    rng = np.random.default_rng(14)
    base = []
    for k in range(64):                                     # odd rows: an impulse of 20 000 to 30 000 every 150 to 400 samples
        at = np.cumsum(rng.integers(150, 400, 16))
        imp = [[int(p), float(rng.uniform(20000, 30000) * rng.choice([-1, 1]))] for p in at[at < n]] if k % 2 else []
        base.append(synth.nb_audio(n, seed=k, impulses=imp))
    base = np.stack(base)
    for C in [int(c) for c in a.channels.split(",")]:
        x = rows_on_device(torch, base, C)
        y = torch.empty_like(x)
        for run in range(a.runs):
            p = nb.NbProcessor(C, nb.nb_config(nb_setting=a.setting), stream=s.cuda_stream)
            ms = timed(torch, lambda: p.process_frames(x, y), a.calls, WARMUP)
            before = p.state()[1].astype(np.int64)
            p.process_frames(x, y)
            places = p.state()[1].astype(np.int64) - before
            p.close()
            emit({"workload": f"nb frames: {F} frames of 128 samples a call, voiced audio, impulses on every second channel, setting {a.setting}",
                  "level": "nb_frames", "channels": C, "frames_per_call": F, "calls": a.calls, "warmup_calls": WARMUP, "run": run,
                  "ms_per_call": round(ms, 4), "frames_per_s": round(C * F / (ms * 1e-3), 0),
                  "ns_per_channel_frame": round(ms * 1e6 / (C * F), 3),
                  "lanes_repairing_share": round(float((places > 0).mean()), 4),
                  "places_per_channel_frame": round(float(places.sum()) / (C * F), 4)}, a.out)
        for level, kw in (("stream_nr", dict()), ("stream_nb_nr", dict(nb_setting=a.setting)), ("stream_nb", dict(nb_setting=a.setting, nr_bypass=1))):
            for run in range(a.runs):
                p = nr.NrProcessor(C, nr.nr_config(width_hz=3200, offset_hz=1700, **kw), stream=s.cuda_stream)
                ms = timed(torch, lambda: p.process(x, y), a.calls, WARMUP)
                p.close()
                emit({"workload": f"12 ksps stream at 3200 Hz, {n} samples ({F} frames) a call: {level}", "level": level, "channels": C,
                      "frames_per_call": F, "calls": a.calls, "warmup_calls": WARMUP, "run": run, "ms_per_call": round(ms, 4),
                      "frames_per_s": round(C * F / (ms * 1e-3), 0), "ns_per_channel_frame": round(ms * 1e6 / (C * F), 3)}, a.out)
        del x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
