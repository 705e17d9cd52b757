"""bench.py --dump-outputs, the writer (CPU): float32 where every value is exact in it, float64 otherwise, and past the size limit
the same share of every array's rows at fixed seeded positions."""
import os

import numpy as np

from bench import step


def test_dump_outputs_dtypes_and_values(tmp_path):
    a = np.arange(-5, 1000, dtype=np.int32)
    big = np.array([0, (1 << 24) - 1, 1 << 24, (1 << 40) + 3], dtype=np.int64)
    rows = np.arange(24, dtype=np.int32).reshape(6, 4)
    step.dump_outputs(str(tmp_path / "d"), dict(a=a, big=big, rows=rows, empty=np.zeros(0, np.int32)))
    assert sorted(os.listdir(tmp_path / "d")) == ["a.npy", "big.npy", "empty.npy", "rows.npy"]
    got = {k: np.load(tmp_path / "d" / f"{k}.npy") for k in ("a", "big", "rows", "empty")}
    assert got["a"].dtype == np.float32 and np.array_equal(got["a"], a)
    assert got["big"].dtype == np.float64 and np.array_equal(got["big"].astype(np.int64), big)
    assert got["rows"].dtype == np.float32 and got["rows"].shape == (6, 4) and np.array_equal(got["rows"], rows)
    assert got["empty"].dtype == np.float32 and got["empty"].shape == (0,)


def test_dump_outputs_samples_past_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(step, "DUMP_BYTES_MAX", 4000)
    x = np.arange(2000, dtype=np.int32)                    # 8000 B as float32
    e = np.arange(2000 * 2, dtype=np.int32).reshape(2000, 2)  # 16000 B
    for d in ("one", "two"):
        step.dump_outputs(str(tmp_path / d), dict(x=x, e=e))
    gx, ge = np.load(tmp_path / "one" / "x.npy"), np.load(tmp_path / "one" / "e.npy")
    assert gx.nbytes + ge.nbytes <= 4000 and len(gx) == len(ge) > 0
    assert np.all(np.diff(gx) > 0) and np.isin(gx, x).all()                  # rows of the array, in order
    assert np.array_equal(ge[:, 1] - ge[:, 0], np.ones(len(ge)))              # whole rows
    assert np.array_equal(gx, np.load(tmp_path / "two" / "x.npy"))            # the same positions every time
    assert np.array_equal(ge, np.load(tmp_path / "two" / "e.npy"))
