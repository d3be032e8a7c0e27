#!/usr/bin/env python3
"""Throughput of the waterfall image against a plain device fill of as many bytes.  Per channel
count, at the panel's 480 x 70 (35 ring lines, each put up to three times) with one frame and one
drawing a call:

  image          uhsdr_wfall_process_lines writing the image, every frame at one centre frequency
  image_shifted  the same with the centre frequency stepping a few pixels every call, so every older
                 line is drawn shifted and padded
  ring_only      the call without an image: the line into the ring
  fill           torch's fill of the image tensor: the yardstick, not the code under test

    python tools/bench_wfall.py [--channels 4096,65536,262144] [--calls 20] [--runs 3] [--out FILE]

Prints one JSON line per run, shape and level: ms per call and the image bytes per second, timed with
device events over the calls after a warm-up.  --out appends the lines to a file."""
import argparse

from benchlib import emit, timed

WARMUP = 5
W, H = 480, 70


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="4096,65536,262144")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import uhsdr_amd as U
    s = torch.cuda.current_stream()
    cfg = U.wfall_config(width=W, height=H, vert_step_size=1, color_scheme=2, magnify=1)
    gen = torch.Generator(device="cuda").manual_seed(19)
    for C in [int(c) for c in a.channels.split(",")]:
        w = U.Waterfall(C, cfg, stream=s.cuda_stream)
        lines = torch.randint(0, 64, (C, 1, W), dtype=torch.uint8, device="cuda", generator=gen)
        image = torch.empty((C, H, W), dtype=torch.int16, device="cuda")
        still = torch.full((C, 1), 7100000, dtype=torch.int32, device="cuda")
        # 350 Hz is 7 pixels of 50 Hz: eight steps up, then back
        moving = [torch.full((C, 1), 7100000 + 350 * k, dtype=torch.int32, device="cuda") for k in range(8)]
        turn = [0]

        def shifted():
            turn[0] += 1
            w.process_lines(lines, moving[turn[0] % 8], image=image)

        def line(level, run, ms):
            emit({"workload": f"waterfall image {W} x {H}, one frame and one drawing a call: {level}", "level": level, "channels": C,
                  "image_bytes_per_call": C * H * W * 2, "calls": a.calls, "warmup_calls": WARMUP, "run": run, "ms_per_call": round(ms, 4),
                  "image_gb_per_s": round(C * H * W * 2 / (ms * 1e-3) / 1e9, 1)}, a.out)

        for _ in range(2 * w.plan.wfall_size * (w.plan.repeat + 1)):      # a full ring before anything is timed
            w.process_lines(lines, still)
        for run in range(a.runs):
            line("image", run, timed(torch, lambda: w.process_lines(lines, still, image=image), a.calls, WARMUP))
            line("image_shifted", run, timed(torch, shifted, a.calls, WARMUP))
            line("ring_only", run, timed(torch, lambda: w.process_lines(lines, still), a.calls, WARMUP))
            line("fill", run, timed(torch, lambda: image.fill_(0x1234), a.calls, WARMUP))
        w.close()
        del lines, image, still, moving
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
