"""What the module bench tools (tools/bench_*.py) share: the device-event timer in the two forms
they use, the tiling of host rows over the channels, and the JSON line.  Importing it puts the
repository root on sys.path."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _start(torch):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    return s, e0, e1


def _stop(torch, s, e0, e1):
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(torch, call, calls, warmup):
    """ms per call over `calls` calls on the current stream, after `warmup` calls and a synchronize"""
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ev = _start(torch)
    for _ in range(calls):
        call()
    return _stop(torch, *ev) / calls


def timed_second_pass(torch, prepare, run, calls):
    """ms per call of a pass of `calls` calls (run()), each pass behind prepare() (a reset, the text):
    the whole pass runs twice and the second one counts"""
    for _ in range(2):                         # pass 0 warms up
        prepare()
        ev = _start(torch)
        run()
        ms = _stop(torch, *ev) / calls
    return ms


def rows_on_device(torch, base, channels):
    """host rows [k][n] tiled over `channels` device rows, row c holding base[c % k]"""
    t = torch.from_numpy(np.ascontiguousarray(base)).cuda()
    return t.repeat((channels + len(base) - 1) // len(base), 1)[:channels].contiguous()


def emit(line, out=None):
    """print the JSON line; append it to the file `out` if there is one"""
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")
