#!/usr/bin/env python3
"""Throughput of the stand-alone BPSK decoder (uhsdr_psk_process, kernel psk_decode) on BPSK125
input: the speed-2 fixture streams (tests/golden/psk_*.npz) tiled over the channels, a different
case on neighbouring lanes, fed in calls of --samples 12 ksps samples.

    python tools/bench_psk.py [--channels 65536] [--samples 512] [--calls 40] [--rtty]

Prints one JSON line: ms per call and channel-samples per second, timed with device events over
the calls after one warm-up pass, plus the host decoder's rate on one thread for scale.  --rtty
adds the RTTY decoder's time on the same input in the same process, for context (its filters run
on every sample whatever the data; tools/bench_rtty.py is its own benchmark)."""
import argparse
import glob
import os
import time

import numpy as np

from benchlib import ROOT, emit, rows_on_device, timed_second_pass


def timed(torch, dec, pieces):
    def run():
        for p in pieces:
            dec.process(p)
    return timed_second_pass(torch, dec.reset, run, len(pieces))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--rtty", action="store_true")
    a = ap.parse_args()
    import torch
    from uhsdr_amd import psk, rtty, synth
    files = sorted(f for f in glob.glob(os.path.join(ROOT, "tests", "golden", "psk_*.npz")) if "psk_chain_" not in f)
    cases = [g["audio"] for g in map(synth.psk_fixture, files) if g["speed"] == psk.SPEED_125 and len(g["audio"]) < 100000]
    need = a.samples * a.calls
    rows = np.stack([np.resize(s, need) for s in cases])
    C = a.channels
    pieces = [rows_on_device(torch, rows[:, k * a.samples:(k + 1) * a.samples], C) for k in range(a.calls)]
    s = torch.cuda.current_stream()
    dec = psk.PskDecoder(C, psk.SPEED_125, capacity=64, stream=s.cuda_stream)
    ms = timed(torch, dec, pieces)
    chars = int(dec.read()[1].astype(np.int64).sum())
    host = psk.PskDecoder(len(rows), psk.SPEED_125, capacity=64, host=True)
    t0 = time.perf_counter()
    host.process(np.ascontiguousarray(rows))
    host_ns = (time.perf_counter() - t0) * 1e9 / rows.size
    out = {"workload": "psk_decode: varicode-to-text, fixture streams tiled over the lanes", "channels": C,
           "samples_per_call": a.samples, "calls": a.calls, "ms_per_call": round(ms, 4),
           "channel_samples_per_s": round(C * a.samples / (ms * 1e-3), 0),
           "ns_per_channel_sample": round(ms * 1e6 / (C * a.samples), 5),
           "characters": chars, "host_ns_per_channel_sample_1_thread": round(host_ns, 1)}
    if a.rtty:
        rdec = rtty.RttyDecoder(C, rtty.SHIFT_170, rtty.SPEED_45, rtty.STOP_1_5, 0, capacity=64, stream=s.cuda_stream)
        out["rtty_ms_per_call_same_process"] = round(timed(torch, rdec, pieces), 4)
    emit(out)


if __name__ == "__main__":
    main()
