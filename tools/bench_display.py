#!/usr/bin/env python3
"""Throughput of the display stage against what a host had before it: the spectrum call that writes
the magnitudes and averages for the host to scale, resample and colour.  Per channel count, at
fft_len 512 -> width 480 and --frames input frames a call (4 display frames at the default;
uhsdr_amd.synth.ssb_iq, 64 different rows tiled over the channels):

  display_frames        uhsdr_display_process_avg alone on stored averages (the frames the call completes)
  spectrum_mag_avg      uhsdr_spectrum_process writing mag and avg (the yardstick: what a host has today)
  fused_display_only    the same call with a display attached, mag and avg null: 3 bytes per column out
  fused_meter_display   the same call with meter and display, mag and avg null

    python tools/bench_display.py [--channels 4096,65536,262144] [--frames 2048] [--calls 20] [--runs 3] [--out FILE]

Prints one JSON line per run, shape and level: ms per call and display frames per second, timed with
device events over the calls after a warm-up.  --out appends the lines to a file."""
import argparse

import numpy as np

from benchlib import emit, timed

WARMUP = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="4096,65536,262144")
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import uhsdr_amd as U
    from uhsdr_amd import display, meter, synth
    L, N = 512, a.frames
    s = torch.cuda.current_stream()
    base = torch.from_numpy(synth.ssb_iq(np.arange(64), 7, N)).cuda()
    cfg = U.default_spectrum_config(fft_len=L)
    dcfg = U.display_config(fft_len=L)
    mcfg = U.meter_config(fft_len=L, dmod_mode=U.DEMOD_AM, filter_path=2, tune_old=7100000)
    kinds = {np.uint16: torch.int16, np.uint8: torch.uint8, np.float32: torch.float32}
    for C in [int(c) for c in a.channels.split(",")]:
        iq = base.repeat((C + 63) // 64, 1, 1)[:C].contiguous()
        spec = U.Spectrum(cfg, channels=C, frames=N, stream=s.cuda_stream)
        F = spec.frames_out
        mag = torch.empty(spec.out_shape, dtype=torch.float32, device="cuda")
        avg = torch.empty(spec.out_shape, dtype=torch.float32, device="cuda")
        d = U.Display(C, dcfg, stream=s.cuda_stream)
        m = U.Meter(C, mcfg, stream=s.cuda_stream)
        rows = {name: torch.empty(d.row_shape(name, F), dtype=kinds[dt], device="cuda") for name, dt in display.OUTPUTS}
        mrows = {name: torch.empty((C, F), dtype=torch.float32 if dt is np.float32 else torch.int32, device="cuda") for name, dt in meter.OUTPUTS}
        edge = torch.zeros((C, F), dtype=torch.float32, device="cuda")
        spec.process(iq, mag, avg)              # averages for display_frames to work on
        torch.cuda.synchronize()

        def line(level, run, ms):
            emit({"workload": f"display stage, fft_len {L} -> width {d.width}, {N} input frames ({F} display frames) a call: {level}",
                  "level": level, "channels": C, "frames_per_call": N, "display_frames_per_call": F, "calls": a.calls, "warmup_calls": WARMUP,
                  "run": run, "ms_per_call": round(ms, 4), "display_frames_per_s": round(C * F / (ms * 1e-3), 0),
                  "ns_per_channel_frame": round(ms * 1e6 / (C * F), 3)}, a.out)

        for run in range(a.runs):
            spec.set_display(None)
            spec.set_meter(None)
            line("display_frames", run, timed(torch, lambda: d.process_avg(avg, edge, **rows), a.calls, WARMUP))
            line("spectrum_mag_avg", run, timed(torch, lambda: spec.process(iq, mag, avg), a.calls, WARMUP))
            spec.set_display(d, **rows)
            line("fused_display_only", run, timed(torch, lambda: spec.process(iq, None, None), a.calls, WARMUP))
            spec.set_meter(m, **mrows)
            line("fused_meter_display", run, timed(torch, lambda: spec.process(iq, None, None), a.calls, WARMUP))
        spec.close()
        d.close()
        m.close()
        del iq, mag, avg, rows, mrows, edge
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
