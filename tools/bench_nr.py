#!/usr/bin/env python3
"""Throughput of the spectral noise reduction on voiced / keyed signals in noise
(uhsdr_amd.synth.nr_audio, 64 different rows tiled over the channels): the frame stage alone
(uhsdr_nr_process_frames, kernel nr_frames, --frames frames of 128 samples a call at 6 ksps) and
the 12 ksps stream around it (uhsdr_nr_process: decimator, frames, FIFO, interpolator; the same
number of frames a call, so 256 * frames input samples).

    python tools/bench_nr.py [--channels 65536] [--frames 16] [--calls 50] [--runs 3] [--out FILE]

Prints one JSON line per run and level: ms per call and frames per second, timed with device events
over the calls after a warm-up of 24 calls (past the 20-frame start-up, so the timed calls run the
noise reduction proper); --out appends the lines to a file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP = 24


def rows_on_device(torch, base, channels):
    t = torch.from_numpy(np.ascontiguousarray(base)).cuda()
    return t.repeat((channels + len(base) - 1) // len(base), 1)[:channels].contiguous()


def timed(torch, call, calls):
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(calls):
        call()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from uhsdr_amd import nr, synth
    C, F = a.channels, a.frames
    s = torch.cuda.current_stream()
    lines = []
    for level, n, rate in (("frames", F * nr.FRAME, 6000.0), ("stream", 2 * F * nr.FRAME, 12000.0)):
        base = np.stack([synth.nr_audio(n, rate=rate, snr_db=-3.0 + 0.36 * k, seed=k) for k in range(64)])
        x = rows_on_device(torch, base, C)
        y = torch.empty_like(x)
        for run in range(a.runs):
            p = nr.NrProcessor(C, nr.nr_config(), stream=s.cuda_stream)
            call = (lambda: p.process_frames(x, y)) if level == "frames" else (lambda: p.process(x, y))
            ms = timed(torch, call, a.calls)
            nn = p.state()[1]
            p.close()
            lines.append({"workload": f"nr {level}: {F} frames of 128 samples a call at 6 ksps, signals in noise tiled over the channels",
                          "level": level, "channels": C, "frames_per_call": F, "calls": a.calls, "warmup_calls": WARMUP, "run": run,
                          "ms_per_call": round(ms, 4), "frames_per_s": round(C * F / (ms * 1e-3), 0),
                          "ns_per_channel_frame": round(ms * 1e6 / (C * F), 3),
                          "realtime_channels_at_6ksps": round(C * F / (ms * 1e-3) / (6000.0 / nr.FRAME), 0),
                          "nn_values": sorted(set(nn.tolist()))})
            print(json.dumps(lines[-1]), flush=True)
        del x, y
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
