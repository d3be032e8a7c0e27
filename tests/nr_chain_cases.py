"""The recordings of the firmware's noise reduction and blanker inside its receive chain
(tests/golden/nrchain_<case>.npz, tools/nr/make_nr_chain_golden.py): two channels per case, two
recordings of one configuration.  The files are nrchain_*, not nr_chain_*: tests/nr_cases.py takes
every nr_*.npz for a stand-alone noise-reduction case."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["ssb_wide", "ssb_narrow", "nb_nr", "nb", "cw", "notch", "mchf", "digi"]
_cache = {}


def load_case(name):
    """the recording, read once and shared; nobody writes to its arrays"""
    if name not in _cache:
        d = np.load(os.path.join(GOLDEN, f"nrchain_{name}.npz"))
        g = {k: d[k] for k in d.files if k not in ("args", "nr", "text")}
        g["name"] = name
        g["args"] = json.loads(str(d["args"]))
        g["nr"] = json.loads(str(d["nr"]))
        if "text" in d.files:
            g["text"] = str(d["text"])
        for v in g.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = g
    return _cache[name]


def nr_cfg(g, **kw):
    from uhsdr_amd import nr
    return nr.nr_config(**dict(g["nr"], **kw))


def same_bits(a, b):
    """bit for bit, two NaNs equal"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
