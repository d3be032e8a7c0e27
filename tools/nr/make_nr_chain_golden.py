#!/usr/bin/env python3
"""Record tests/golden/nrchain_<case>.npz: the firmware's noise reduction and blanker inside its
receive chain.

Builds tools/nr/nr_chain_capture.c with the reference harness and its own main (nr.mk and
nr_chain.mk, through oracle/ref/Makefile; once more with the mcHF board's macros for the mcHF case)
into a git-ignored or outside directory, generates each case's I/Q with uhsdr_amd.synth, runs one
process per channel (the driver's state is global) and stores, per case, two channels -- two
recordings of one configuration, so a test can put different ones on neighbouring channels:

  args json                 the harness' key=value arguments (uhsdr_amd._abi.config_from_ref_args)
  nr json                   the stage's uhsdr_nr_config fields: alpha, asnr, width, power_threshold_int,
                            width_hz, offset_hz (FilterInfo[id].width and the path's offset),
                            nb_setting, nr_bypass
  iq int32 [2][n][2]        the I/Q frames
  nr_in, nr_out f32 [2][n/4]   each 8-sample block entering and leaving
                            AudioDriver_RxProcessorNoiseReduction (12 ksps)
  audio f32 [2][n]          adb.a_buffer[1] after each call
  dst int32 [2][n][2], a0 f32 [2][n]   codec frames and adb.a_buffer[0] (the mcHF case)
  tap f32 [2][n/4]          the sample handed to the modem (the DIGI case)
  text                      the DIGI case's message

and asserts what each recording is for.  AudioNr_HandleNoiseReduction runs once after every 32-frame
block: a main loop that never falls behind.

  python3 tools/nr/make_nr_chain_golden.py [--check] [--out DIR] [--ref /root/reference/mchf-eclipse]
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recording  # noqa: E402
from uhsdr_amd import synth  # noqa: E402

ROOT = recording.ROOT
FRAMES_12K, FRAMES_6K = 15360, 30720           # 30 NR frames of 128 samples at the frames' rate
LATENCY = 256                                   # two frames of the output FIFO
NB_LAG = 13                                     # the blanker's own delay
STARTUP = 20                                    # frames the noise reduction passes unchanged
DIGI_TEXT = "RYRY CQ DE UHSDR K"
DEMOD_USB, DEMOD_LSB, DEMOD_CW, DEMOD_DIGI = 0, 1, 2, 6
STRENGTH = 50


def alpha_from_strength(s):
    """audio_driver.c:1195, 0.799 + ((float32_t)nr_strength / 1000.0) assigned to a float"""
    return float(np.float32(0.799 + float(np.float32(s)) / 1000.0))


def impulses(iq, channel):
    """full-scale clicks of one frame, every 2311 + 97 * channel frames, alternating in sign"""
    out = iq.copy()
    pos = np.arange(1500 + 311 * channel, iq.shape[0], 2311 + 97 * channel)
    out[pos, 0] = (np.where(np.arange(len(pos)) % 2 == 0, 30000, -30000)).astype(np.int32) << 16
    out[pos, 1] = 0
    return out


def cases():
    def case(name, path, mode, kind="ssb", dsp=1, nb_setting=0, board=0, clicks=False, noise=400.0, **args):
        a = dict(mode=mode, path=path)
        if dsp:
            a["dsp"] = dsp
        if board:
            a["board"] = board
        a.update(args)
        return dict(name=name, path=path, kind=kind, args=a, nb_setting=nb_setting, nr_on=bool(dsp & 1), board=board, clicks=clicks,
                    noise=noise)
    return [
        case("ssb_wide", 48, DEMOD_USB),
        case("ssb_narrow", 35, DEMOD_LSB),
        case("nb_nr", 48, DEMOD_USB, nb_setting=15, clicks=True),      # the I/Q and setting of "nb", whose check shows the repairs
        case("nb", 48, DEMOD_USB, dsp=0, nb_setting=15, clicks=True),
        case("cw", 4, DEMOD_CW, kind="cw", cwthresh=1000),
        case("notch", 48, DEMOD_USB, dsp=5),
        case("mchf", 48, DEMOD_LSB, board=1, spkr=30),
        case("digi", 48, DEMOD_DIGI, kind="rtty", noise=200.0),
    ]


def make_iq(c, channel, n):
    if c["kind"] == "cw":
        iq = synth.cw_iq([channel], 0, n, noise_sigma=c["noise"])[0]
    elif c["kind"] == "rtty":
        iq = synth.rtty_iq([channel], 0, n, DIGI_TEXT, noise_sigma=c["noise"], lead=2400)[0]
    else:
        iq = synth.ssb_iq([channel], 0, n, noise_sigma=c["noise"], lsb=c["args"]["mode"] == DEMOD_LSB)[0]
    iq = np.ascontiguousarray(iq, dtype=np.int32)
    return impulses(iq, channel) if c["clicks"] else iq


def filter_of(rec, c, tmp):
    """FilterInfo[ts.filters_p->id].width and ts.filters_p->offset of the case, as the compiled reference holds
    them: the recorder writes both at the stage's first block (64 frames of silence are enough)"""
    fin, finfo = os.path.join(tmp, "probe.iq"), os.path.join(tmp, "probe.info")
    np.zeros((64, 2), np.int32).tofile(fin)
    env = dict(os.environ, NRC_NB_SETTING=str(c["nb_setting"]), NRC_INFO_LOG=finfo)
    subprocess.run([rec, f"in={fin}", "n=64"] + [f"{k}={v}" for k, v in c["args"].items()], check=True, env=env)
    width, offset = (int(x) for x in open(finfo).read().split())
    os.remove(finfo)
    return width, offset


def main():
    a = recording.parse_args()
    out = recording.build(a, ["nr", "nr/nr_chain"], ["nr_chain"])
    mchf_out = os.path.join(out, "mchf")
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle", "ref"), "-f", "Makefile", "-f", os.path.join(ROOT, "tools", "nr", "nr.mk"),
                    "-f", os.path.join(ROOT, "tools", "nr", "nr_chain.mk"), f"OUT={mchf_out}", f"REF={a.ref}",
                    f"VARIANT_CFLAGS=-include {os.path.join(ROOT, 'oracle', 'ref', 'mchf_board.h')}", "-j8", "nr_chain"],
                   check=True, stdout=subprocess.DEVNULL)
    writer = recording.Recorder(a)

    with tempfile.TemporaryDirectory() as tmp:
        for c in cases():
            rec = os.path.join(mchf_out if c["board"] else out, "nr_chain")
            width_hz, offset_hz = filter_of(rec, c, tmp)
            decimated = width_hz < 2701
            n = FRAMES_6K if decimated else FRAMES_12K
            nr = dict(alpha=alpha_from_strength(STRENGTH), asnr=30, width=4, power_threshold_int=40, width_hz=width_hz,
                      offset_hz=offset_hz, nb_setting=c["nb_setting"], nr_bypass=int(not c["nr_on"]))
            got = dict(iq=[], nr_in=[], nr_out=[], audio=[], dst=[], a0=[], tap=[])
            for channel in (0, 1):
                iq = make_iq(c, channel, n)
                f = {k: os.path.join(tmp, f"{c['name']}{channel}.{k}") for k in ("iq", "in", "out", "tap", "a", "dst", "a0")}
                iq.tofile(f["iq"])
                env = dict(os.environ, NRC_NB_SETTING=str(c["nb_setting"]), NRC_STRENGTH=str(STRENGTH), NRC_ASNR=str(nr["asnr"]),
                           NRC_WIDTH=str(nr["width"]), NRC_THRESHOLD=str(nr["power_threshold_int"]),
                           NRC_RTTY=str(int(c["kind"] == "rtty")), NRC_IN_LOG=f["in"], NRC_OUT_LOG=f["out"], NRC_TAP_LOG=f["tap"])
                subprocess.run([rec, f"in={f['iq']}", f"n={n}", f"out_a={f['a']}", f"out_dst={f['dst']}", f"out_a0={f['a0']}"]
                               + [f"{k}={v}" for k, v in c["args"].items()], check=True, env=env)
                x, y = np.fromfile(f["in"], dtype=np.float32), np.fromfile(f["out"], dtype=np.float32)
                audio = np.fromfile(f["a"], dtype=np.float32)
                assert len(x) == n // 4 and len(y) == n // 4 and len(audio) == n, f"{c['name']}: {len(x)} in, {len(y)} out, {len(audio)} audio"
                assert np.isfinite(y).all() and np.isfinite(audio).all(), c["name"]
                # what the recording is for
                step = 2 if decimated else 1                    # 12 ksps samples per sample of a frame
                first = int(np.argmax(y != 0))
                # the latency the recording shows: two frames at the frames' rate, silence until then
                assert LATENCY * step <= first < LATENCY * step + 128, f"{c['name']}: first output at {first}"
                after = (STARTUP + 4) * 128 * step
                assert len(y) >= after + 4 * 128 * step, c["name"]
                lag = LATENCY * step + (NB_LAG * step if c["nb_setting"] else 0)
                delayed, tail = x[after - lag:len(x) - lag], y[after:]
                changed = float(np.mean(delayed != tail))
                if c["nr_on"]:
                    assert changed > 0.9, f"{c['name']}: the noise reduction changed {changed:.3f} of the samples after start-up"
                else:
                    assert 0.0 < changed < 0.5, f"{c['name']}: the blanker changed {changed:.3f} of the samples"
                assert np.abs(audio[n // 2:]).max() > 1.0, f"{c['name']}: silent audio"
                got["iq"].append(iq); got["nr_in"].append(x); got["nr_out"].append(y); got["audio"].append(audio)
                if c["board"]:
                    got["dst"].append(np.fromfile(f["dst"], dtype=np.int32).reshape(n, 2))
                    got["a0"].append(np.fromfile(f["a0"], dtype=np.float32))
                if c["kind"] == "rtty":
                    tap = np.fromfile(f["tap"], dtype=np.float32)
                    assert len(tap) == n // 4, c["name"]
                    got["tap"].append(tap)
                print(f"{c['name']:11s} ch {channel}  {n:6d} frames  width {width_hz:4d} offset {offset_hz:4d}  first output at {first:4d}  "
                      f"changed {changed:.3f}")
            arrays = {k: np.stack(v) for k, v in got.items() if v}
            if c["kind"] == "rtty":
                arrays["text"] = np.array(DIGI_TEXT)
            writer.save(f"nrchain_{c['name']}.npz", args=np.array(json.dumps(c["args"])), nr=np.array(json.dumps(nr)), **arrays)
    writer.finish()


if __name__ == "__main__":
    main()
