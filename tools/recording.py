"""What the fixture makers (tools/*/make_*_golden.py) share: the command line, the build of a
module's recorders against the reference objects, and the one place a recording is written.

    a = recording.parse_args()
    out = recording.build(a, ["nr"], ["nr_driver", "nr_stream"])
    writer = recording.Recorder(a)
    word = writer.save("nr_tables.npz", sqrt_hann_256=window, ...)      # "unchanged" or "NEW"
    writer.finish()

A recording equals its file when the key sets are equal and every array has the file's dtype,
shape and bytes.  An equal recording leaves the file untouched; another one is written, or under --check only
noted, and finish() then exits non-zero naming every file that would change."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "oracle", "_ref"), help="build directory (git-ignored or outside)")
    ap.add_argument("--ref", default="/root/reference/mchf-eclipse")
    ap.add_argument("--golden", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--check", action="store_true", help="fail where a file would change instead of writing it")
    return ap.parse_args()


def build(args, fragments, targets):
    """make `targets` by oracle/ref/Makefile plus tools/<m>/<m>.mk for each m of `fragments` (tools/<d>/<f>.mk for one
    given as "<d>/<f>"); returns the build directory"""
    out = os.path.abspath(args.out)
    frags = [x for m in fragments for x in ("-f", os.path.join(ROOT, "tools", m + ".mk" if "/" in m else os.path.join(m, m + ".mk")))]
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle", "ref"), "-f", "Makefile", *frags, f"OUT={out}", f"REF={args.ref}", "-j8", *targets],
                   check=True, stdout=subprocess.DEVNULL)
    return out


def same(path, arrays):
    if not os.path.exists(path):
        return False
    with np.load(path) as old:
        return set(old.files) == set(arrays) and all(
            old[k].dtype == np.asarray(v).dtype and old[k].shape == np.shape(v) and old[k].tobytes() == np.asarray(v).tobytes()
            for k, v in arrays.items())


class Recorder:
    def __init__(self, args):
        self.golden, self.check, self.saved, self.changed = args.golden, args.check, 0, []

    def save(self, name, **arrays):
        path = os.path.join(self.golden, name)
        self.saved += 1
        if same(path, arrays):
            return "unchanged"
        self.changed.append(path)
        if not self.check:
            np.savez_compressed(path, **arrays)
        return "NEW"

    def finish(self):
        if self.check and self.changed:
            sys.exit("recordings differ from the committed files:\n  " + "\n  ".join(self.changed))
        print(f"{self.saved} recordings, {self.saved - len(self.changed)} unchanged" + "".join(f"\n  wrote {p}" for p in self.changed))
