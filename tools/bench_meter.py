#!/usr/bin/env python3
"""Throughput of the signal meter against what a host had before it: the spectrum call that writes
the magnitudes for the host to reduce.  Per channel count, at fft_len 256 and --frames input frames a
call (uhsdr_amd.synth.ssb_iq, 64 different rows tiled over the channels), in AM so that SNAP runs:

  spectrum_mag        uhsdr_spectrum_process writing mag (the yardstick)
  fused_meter_only    the same call with a meter attached, mag and avg null: six values per frame out
  fused_meter_all     the same call with the meter, mag and avg
  meter_frames        uhsdr_meter_process_mag alone on stored magnitudes (the frames the call completes)

    python tools/bench_meter.py [--channels 4096,65536,262144] [--frames 1024] [--calls 20] [--runs 3] [--out FILE]

Prints one JSON line per run, shape and level: ms per call and display frames per second, timed with
device events over the calls after a warm-up.  --out appends the lines to a file."""
import argparse

import numpy as np

from benchlib import emit, timed

WARMUP = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="4096,65536,262144")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import uhsdr_amd as U
    from uhsdr_amd import meter, synth
    L, N = 256, a.frames
    s = torch.cuda.current_stream()
    base = torch.from_numpy(synth.ssb_iq(np.arange(64), 7, N)).cuda()
    cfg = U.default_spectrum_config(fft_len=L)
    mcfg = U.meter_config(fft_len=L, dmod_mode=U.DEMOD_AM, filter_path=2, tune_old=7100000)
    for C in [int(c) for c in a.channels.split(",")]:
        iq = base.repeat((C + 63) // 64, 1, 1)[:C].contiguous()
        spec = U.Spectrum(cfg, channels=C, frames=N, stream=s.cuda_stream)
        F = spec.frames_out
        mag = torch.empty(spec.out_shape, dtype=torch.float32, device="cuda")
        avg = torch.empty(spec.out_shape, dtype=torch.float32, device="cuda")
        m = U.Meter(C, mcfg, stream=s.cuda_stream)
        rows = {name: torch.empty((C, F), dtype=torch.float32 if dt is np.float32 else torch.int32, device="cuda") for name, dt in meter.OUTPUTS}

        def line(level, run, ms):
            emit({"workload": f"signal meter, fft_len {L}, {N} input frames ({F} display frames) a call, AM passband of {m.plan.ubin - m.plan.lbin + 1} bins: {level}",
                  "level": level, "channels": C, "frames_per_call": N, "display_frames_per_call": F, "calls": a.calls, "warmup_calls": WARMUP,
                  "run": run, "ms_per_call": round(ms, 4), "display_frames_per_s": round(C * F / (ms * 1e-3), 0),
                  "ns_per_channel_frame": round(ms * 1e6 / (C * F), 3)}, a.out)

        for run in range(a.runs):
            spec.set_meter(None)
            line("spectrum_mag", run, timed(torch, lambda: spec.process(iq, mag, None), a.calls, WARMUP))
            spec.set_meter(m, **rows)
            line("fused_meter_only", run, timed(torch, lambda: spec.process(iq, None, None), a.calls, WARMUP))
            line("fused_meter_all", run, timed(torch, lambda: spec.process(iq, mag, avg), a.calls, WARMUP))
            spec.set_meter(None)
            line("meter_frames", run, timed(torch, lambda: m.process_mag(mag, **rows), a.calls, WARMUP))
        spec.close()
        m.close()
        del iq, mag, avg, rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
