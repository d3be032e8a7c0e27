#!/usr/bin/env python3
"""Throughput of the stand-alone RTTY and BPSK modulators (uhsdr_rttymod_process, kernel
rttymod_gen; uhsdr_pskmod_process, kernel pskmod_gen): the fixtures' texts in rotation over the
channels, a different text on neighbouring lanes and every sixth queue empty, generated in calls of
--samples 48 ksps samples into one int16 [C][samples] buffer.

    python tools/bench_digimod.py [--channels 4096,65536,262144] [--samples 2048] [--calls 40]

Prints one JSON line per modulator and channel count: ms per call, channel-samples per second and
the output's bytes per second, timed with device events over the calls after one warm-up pass, plus
the host modulator's rate on one thread for scale."""
import argparse
import time

import numpy as np

from benchlib import emit, timed_second_pass

TEXTS = [b"RYRY CQ DE UHSDR K", b"A1B2C3-D4?E5", b"the quick brown fox 0123456789", b"CQ CQ de UHSDR, Pse k (QSL?) #7", b"599 73\r\n", b""]


def make(kind, channels, host=False, stream=None):
    from uhsdr_amd import digimod, psk
    if kind == "rtty":
        return digimod.RttyModulator(channels, capacity=64, host=host, stream=stream)
    return digimod.PskModulator(channels, psk.SPEED_125, capacity=64, host=host, stream=stream)


def timed(torch, mod, audio, calls, texts):
    def prepare():
        mod.reset()
        mod.put_text(texts)

    def run():
        for _ in range(calls):
            mod.process(audio)
    return timed_second_pass(torch, prepare, run, calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="4096,65536,262144")
    ap.add_argument("--samples", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=40)
    a = ap.parse_args()
    import torch
    s = torch.cuda.current_stream()
    for kind in ("rtty", "psk"):
        host = make(kind, len(TEXTS), host=True)
        host.put_text(TEXTS)
        t0 = time.perf_counter()
        host.generate(a.samples * a.calls)
        host_rate = len(TEXTS) * a.samples * a.calls / (time.perf_counter() - t0)
        host.close()
        for C in (int(x) for x in a.channels.split(",")):
            texts = [TEXTS[c % len(TEXTS)] for c in range(C)]
            mod = make(kind, C, stream=s.cuda_stream)
            audio = torch.zeros((C, a.samples), dtype=torch.int16, device="cuda")
            ms = timed(torch, mod, audio, a.calls, texts)
            took = int(mod.consumed().astype(np.int64).sum())
            mod.close()
            del audio
            emit(dict(bench="digimod", kind=kind, channels=C, samples=a.samples, calls=a.calls, ms_per_call=round(ms, 4),
                      channel_samples_per_s=round(C * a.samples / ms * 1e3), out_gbytes_per_s=round(2 * C * a.samples / ms / 1e6, 2),
                      realtime_channels=round(C * a.samples / ms * 1e3 / 48000), characters_taken=took,
                      host_samples_per_s=round(host_rate)))


if __name__ == "__main__":
    main()
