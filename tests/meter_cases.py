"""The signal-meter fixtures (tests/golden/meter_*.npz, recorded from the reference firmware by
tools/meter/make_meter_golden.py): the configuration, the frames of FFT_MagData (taken from the
spectrum recording the case names, or stored), checked against the recorded crc32, the six outputs
per channel and frame, and Lbin / Ubin / posbin as the firmware computed them.  Loaded once and
shared; nothing here is modified by a test.  What the set as a whole must show is asserted by
check_set()."""
import functools
import glob
import json
import os
import zlib

import numpy as np

from uhsdr_amd import meter

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("meter_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "meter_*.npz"))
               if not p.endswith("meter_tables.npz"))
SPEC_CASES = [n for n in CASES if n.startswith("p48_")]       # frames of a spec_*.npz recording
OUTPUTS = [name for name, _ in meter.OUTPUTS]
DEMOD_CW, DEMOD_AM, DEMOD_SAM, DEMOD_DIGI = 2, 3, 4, 6


def same(a, b):
    """bit for bit, two NaNs equal"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    eq = a.view(np.uint32) == b.view(np.uint32)
    return eq | (np.isnan(a) & np.isnan(b)) if a.dtype == np.float32 else eq


def sample_index(L, j):
    """the bin of FFT_MagData that sd.FFT_Samples[j] is taken from"""
    return (L - 1 - j + L // 2) % L


def config_of(g):
    return meter.meter_config(**g["cfg"])


@functools.lru_cache(maxsize=None)
def load_case(name):
    with np.load(os.path.join(GOLDEN, f"meter_{name}.npz")) as z:
        g = {k: z[k] for k in z.files}
    g["name"] = name
    g["cfg"] = json.loads(str(g.pop("config")))
    source = json.loads(str(g.pop("source")))
    g["spec"] = source.get("spec")
    if g["spec"]:
        with np.load(os.path.join(GOLDEN, f"spec_{g['spec']}.npz")) as z:
            mag, g["iq"], g["spec_args"] = z["mag"], z["iq"], json.loads(str(z["args"]))
        g["spec_frames"] = mag.shape[1]
        g["mag"] = np.ascontiguousarray(mag[:, np.arange(source["frames"]) % mag.shape[1]])
    assert zlib.crc32(g["mag"].tobytes()) == int(g["crc32"]), name
    C, F, L = g["mag"].shape
    g["channels"], g["frames"], g["L"] = C, F, L
    assert L == g["cfg"]["fft_len"] and F >= 8, name
    for k, (out, dt) in enumerate(meter.OUTPUTS):
        assert g[out].shape == (C, F) and g[out].dtype == dt, (name, out)
    lbin, ubin, posbin = (int(x) for x in g["bins"])
    assert 0 <= lbin <= ubin <= L - 1, name
    if name == "cw_onebin":
        assert (lbin, ubin, posbin) == (0, 0, 128) and np.isfinite(g["dbmhz_cur"]).all(), name
    # where SNAP runs the estimate moves, where it does not it stays; no case has its maximum in the last bin
    dmod = g["cfg"]["dmod_mode"]
    carrier = dmod in (DEMOD_AM, DEMOD_SAM) or (dmod == DEMOD_DIGI and g["cfg"]["digital_mode"] == 2)
    g["snap_mode"] = 0 if not g["cfg"]["snap_enable"] else 1 if carrier else 2 if dmod == DEMOD_CW else 0
    snap = g["snap_carrier_freq"]
    for c in range(C):
        runs = np.ones(F, bool) if g["snap_mode"] == 1 else g["cw_signal"][c] != 0 if g["snap_mode"] == 2 else np.zeros(F, bool)
        prev = np.concatenate([[0], snap[c, :-1]])
        assert (snap[c][~runs] == prev[~runs]).all(), name
        if runs.any():
            assert (snap[c][runs] != prev[runs]).any(), name
            s = g["mag"][c][runs][:, [sample_index(L, j) for j in range(lbin, ubin + 1)]] * np.float32(1000)
            s = np.where(s > 0, s, 0)
            maxbin = np.where(s.max(axis=1) > 0, lbin + s.argmax(axis=1), 1)
            assert (maxbin != L - 1).all(), name
    return g


def check_set():
    """at least five S-counts, both branches of the averager pair, -145 on an empty passband"""
    s_counts, rises, falls = set(), 0, 0
    for name in CASES:
        g = load_case(name)
        s_counts |= set(g["s_count"].ravel().tolist())
        with np.errstate(invalid="ignore"):
            d = np.diff(g["dbm"], axis=1)
        rises += int((d > 0).sum())
        falls += int((d < 0).sum())
    assert len(s_counts) >= 5 and rises > 0 and falls > 0, (s_counts, rises, falls)
    z = load_case("zero")
    assert (z["dbm_cur"] == -145).all() and (z["dbmhz_cur"] == -145).all()


def check_rows(g, rows, first=0, frames=None, what=""):
    """rows: the six outputs by name, [C][n] each, computed for the frames from `first` on"""
    n = frames if frames is not None else np.shape(rows[OUTPUTS[0]])[1]
    for out in OUTPUTS:
        got = np.ascontiguousarray(rows[out])[:, :n]
        want = g[out][:, first:first + n]
        bad = np.argwhere(~same(got, want))
        assert len(bad) == 0, (f"{g['name']} {what}: {out} differs at {len(bad)} of {got.size} places, first (channel, frame) "
                               f"{tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}")
