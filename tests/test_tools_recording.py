"""The write path of the fixture makers (tools/recording.py): every module recording under
tests/golden is written, left alone or reported by Recorder.save / finish."""
import argparse
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("recording", os.path.join(ROOT, "tools", "recording.py"))
recording = importlib.util.module_from_spec(spec)
spec.loader.exec_module(recording)

OLD = 1_000_000_000          # an mtime no write of today gives


def arrays():
    return dict(out=np.array([1.5, -0.0, np.nan], np.float32), n=np.int32(3), text=np.array("cq"), crc=np.arange(4, dtype=np.uint32))


def recorder(tmp_path, check=False):
    return recording.Recorder(argparse.Namespace(golden=str(tmp_path), check=check))


def seed(tmp_path, names=("a.npz", "b.npz")):
    """files as an earlier run left them, with their bytes"""
    rec = recorder(tmp_path)
    for name in names:
        assert rec.save(name, **arrays()) == "NEW"
        os.utime(tmp_path / name, (OLD, OLD))
    return {name: (tmp_path / name).read_bytes() for name in names}


def untouched(tmp_path, before):
    return all((tmp_path / n).read_bytes() == b and os.stat(tmp_path / n).st_mtime == OLD for n, b in before.items())


def test_equal_recording_leaves_the_file_alone(tmp_path):
    before = seed(tmp_path)
    rec = recorder(tmp_path)
    assert [rec.save(n, **arrays()) for n in before] == ["unchanged", "unchanged"]
    assert rec.changed == [] and untouched(tmp_path, before)
    rec.finish()
    check = recorder(tmp_path, check=True)
    assert check.save("a.npz", **arrays()) == "unchanged"
    check.finish()                                   # nothing differs: no exit


def changed_value(a):
    a["out"] = np.array([1.5, 0.0, np.nan], np.float32)      # the sign of a zero: equal to ==, other bytes


def changed_dtype(a):
    a["crc"] = a["crc"].astype(np.int64)                     # equal values


def added_key(a):
    a["extra"] = np.uint8(1)


def missing_key(a):
    del a["n"]


@pytest.mark.parametrize("change", [changed_value, changed_dtype, added_key, missing_key])
def test_a_change_rewrites_only_that_file(tmp_path, change):
    before = seed(tmp_path)
    new = arrays()
    change(new)
    rec = recorder(tmp_path)
    assert rec.save("a.npz", **arrays()) == "unchanged" and rec.save("b.npz", **new) == "NEW"
    assert rec.changed == [str(tmp_path / "b.npz")]
    assert untouched(tmp_path, {"a.npz": before["a.npz"]})
    with np.load(tmp_path / "b.npz") as z:
        assert set(z.files) == set(new) and all(z[k].dtype == np.asarray(new[k]).dtype and z[k].tobytes() == np.asarray(new[k]).tobytes()
                                                for k in new)
    rec.finish()                                     # without --check a written file is no failure


def test_missing_file_is_written(tmp_path):
    before = seed(tmp_path, ["a.npz"])
    rec = recorder(tmp_path)
    assert rec.save("c.npz", **arrays()) == "NEW" and rec.changed == [str(tmp_path / "c.npz")]
    assert (tmp_path / "c.npz").exists() and untouched(tmp_path, before)
    assert recorder(tmp_path).save("c.npz", **arrays()) == "unchanged"


@pytest.mark.parametrize("change", [changed_value, changed_dtype, added_key, missing_key])
def test_check_writes_nothing_and_names_the_file(tmp_path, change):
    before = seed(tmp_path)
    new = arrays()
    change(new)
    rec = recorder(tmp_path, check=True)
    assert rec.save("a.npz", **arrays()) == "unchanged" and rec.save("b.npz", **new) == "NEW" and rec.save("c.npz", **arrays()) == "NEW"
    assert untouched(tmp_path, before) and sorted(os.listdir(tmp_path)) == ["a.npz", "b.npz"]
    with pytest.raises(SystemExit) as e:
        rec.finish()
    assert e.value.code not in (None, 0)
    assert str(tmp_path / "b.npz") in str(e.value.code) and str(tmp_path / "c.npz") in str(e.value.code)
    assert str(tmp_path / "a.npz") not in str(e.value.code)
