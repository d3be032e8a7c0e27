#!/usr/bin/env python3
"""Throughput of the stand-alone CW text decoder (uhsdr_cwdec_process, kernel cw_decode) on keyed
input: the blocksize-88 fixture streams (tests/golden/cwtext_*_b88.npz, spikecancel 0) tiled over
the channels, a different case on neighbouring lanes, fed in calls of --blocks CW blocks.

    python tools/bench_cwdec.py [--channels 131072] [--blocks 64] [--calls 60]

Prints one JSON line: ms per call and ns per channel-block, timed with device events over the
calls after one warm-up pass, plus the host decoder's rate on one thread for scale."""
import argparse
import glob
import os
import time

import numpy as np

from benchlib import ROOT, emit, rows_on_device, timed_second_pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=131072)
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--calls", type=int, default=60)
    a = ap.parse_args()
    import torch
    from uhsdr_amd import cwdec
    cases = [np.load(p) for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "cwtext_*_b88.npz")))]
    cases = [z["state"] for z in cases if int(z["spikecancel"]) == 0]
    need = a.blocks * a.calls
    rows = np.stack([np.resize(s, need) for s in cases])
    C = a.channels
    state = rows_on_device(torch, rows, C)
    pieces = [state[:, k * a.blocks:(k + 1) * a.blocks].contiguous() for k in range(a.calls)]
    del state
    s = torch.cuda.current_stream()
    dec = cwdec.CwDecoder(C, 88, 0, 64, stream=s.cuda_stream)

    def run():
        for p in pieces:
            dec.process(p)
    ms = timed_second_pass(torch, dec.reset, run, a.calls)
    chars = int(dec.read()[1].astype(np.int64).sum())
    host = cwdec.CwDecoder(len(rows), 88, 0, 64, host=True)
    t0 = time.perf_counter()
    host.process(np.ascontiguousarray(rows))
    host_ns = (time.perf_counter() - t0) * 1e9 / rows.size
    emit({"workload": "cw_decode: Morse-to-text, fixture streams tiled over the lanes", "channels": C,
          "blocks_per_call": a.blocks, "calls": a.calls, "ms_per_call": round(ms, 4),
          "ns_per_channel_block": round(ms * 1e6 / (C * a.blocks), 4),
          "characters": chars, "host_ns_per_channel_block_1_thread": round(host_ns, 1)})


if __name__ == "__main__":
    main()
