#!/usr/bin/env python3
"""Throughput of the stand-alone RTTY decoder (uhsdr_rtty_process, kernel rtty_decode) on FSK
input: the 170 Hz / 45.45 baud / 1.5 stop bit fixture streams (tests/golden/rtty_*.npz, ATC on)
tiled over the channels, a different case on neighbouring lanes, fed in calls of --samples
12 ksps samples.

    python tools/bench_rtty.py [--channels 65536] [--samples 512] [--calls 40]

Prints one JSON line: ms per call and channel-samples per second, timed with device events over
the calls after one warm-up pass, plus the host decoder's rate on one thread for scale."""
import argparse
import glob
import os
import time

import numpy as np

from benchlib import ROOT, emit, rows_on_device, timed_second_pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--calls", type=int, default=40)
    a = ap.parse_args()
    import torch
    from uhsdr_amd import rtty, synth
    config = (rtty.SHIFT_170, rtty.SPEED_45, rtty.STOP_1_5, 0)
    files = sorted(f for f in glob.glob(os.path.join(ROOT, "tests", "golden", "rtty_*.npz")) if "rtty_chain_" not in f)
    cases = [g["audio"] for g in map(synth.rtty_fixture, files) if g["config"] == config]
    need = a.samples * a.calls
    rows = np.stack([np.resize(s, need) for s in cases])
    C = a.channels
    pieces = [rows_on_device(torch, rows[:, k * a.samples:(k + 1) * a.samples], C) for k in range(a.calls)]
    s = torch.cuda.current_stream()
    dec = rtty.RttyDecoder(C, *config, capacity=64, stream=s.cuda_stream)

    def run():
        for p in pieces:
            dec.process(p)
    ms = timed_second_pass(torch, dec.reset, run, a.calls)
    chars = int(dec.read()[1].astype(np.int64).sum())
    host = rtty.RttyDecoder(len(rows), *config, capacity=64, host=True)
    t0 = time.perf_counter()
    host.process(np.ascontiguousarray(rows))
    host_ns = (time.perf_counter() - t0) * 1e9 / rows.size
    emit({"workload": "rtty_decode: Baudot-to-text, fixture streams tiled over the lanes", "channels": C,
          "samples_per_call": a.samples, "calls": a.calls, "ms_per_call": round(ms, 4),
          "channel_samples_per_s": round(C * a.samples / (ms * 1e-3), 0),
          "ns_per_channel_sample": round(ms * 1e6 / (C * a.samples), 5),
          "characters": chars, "host_ns_per_channel_sample_1_thread": round(host_ns, 1)})


if __name__ == "__main__":
    main()
