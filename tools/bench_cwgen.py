#!/usr/bin/env python3
"""Throughput of the stand-alone CW generator (uhsdr_cwgen_process, kernel cwgen_gen): an iambic B
keyer at 30 wpm, texts in rotation over the channels so that neighbouring lanes key different
characters, every fifth channel squeezed by hand and every sixth idle, generated in calls of
--samples 48 ksps samples into two f32 [C][samples] buffers.

    python tools/bench_cwgen.py [--channels 4096,65536,262144] [--samples 512] [--calls 40]

Prints one JSON line per channel count: ms per call, channel-samples per second and the output's
bytes per second, timed with device events over the calls after one warm-up pass, plus the host
generator's rate on one thread for scale."""
import argparse
import time

import numpy as np

from benchlib import emit, timed_second_pass

TEXTS = [b"CQ CQ DE UHSDR K", b"5NN TU 73", b"the quick brown fox", b"QRZ? PSE AGN", b"", b""]


def keys_for(channels, blocks):
    keys = np.zeros((channels, blocks), np.uint8)
    keys[4::6] = 3          # squeezed; a closed line also empties these channels' queues
    return keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="4096,65536,262144")
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--calls", type=int, default=40)
    a = ap.parse_args()
    import torch
    from uhsdr_amd import cwgen
    blocks = a.samples // cwgen.BLOCK
    s = torch.cuda.current_stream()
    host = cwgen.CwGenerator(len(TEXTS), speed=30, capacity=64, host=True)
    host.put_text(TEXTS)
    t0 = time.perf_counter()
    host.generate(keys_for(len(TEXTS), blocks * a.calls))
    host_rate = len(TEXTS) * a.samples * a.calls / (time.perf_counter() - t0)
    host.close()
    for C in (int(x) for x in a.channels.split(",")):
        texts = [TEXTS[c % len(TEXTS)] for c in range(C)]
        gen = cwgen.CwGenerator(C, speed=30, capacity=64, stream=s.cuda_stream)
        keys = torch.from_numpy(keys_for(C, blocks)).cuda()
        i = torch.zeros((C, a.samples), dtype=torch.float32, device="cuda")
        q = torch.zeros_like(i)

        def prepare():
            gen.reset()
            gen.put_text(texts)

        def run():
            for _ in range(a.calls):
                gen.process(keys, i, q)
        ms = timed_second_pass(torch, prepare, run, a.calls)
        active = float((gen.flags() & 1).mean())
        took = int(gen.consumed().astype(np.int64).sum())
        gen.close()
        del i, q, keys
        emit(dict(bench="cwgen", channels=C, samples=a.samples, calls=a.calls, ms_per_call=round(ms, 4),
                  channel_samples_per_s=round(C * a.samples / ms * 1e3), out_gbytes_per_s=round(8 * C * a.samples / ms / 1e6, 2),
                  realtime_channels=round(C * a.samples / ms * 1e3 / 48000), keyed_fraction_last_call=round(active, 3),
                  characters_taken=took, host_samples_per_s=round(host_rate)))


if __name__ == "__main__":
    main()
