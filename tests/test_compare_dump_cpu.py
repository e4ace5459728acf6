"""tools/compare_dump.py --npy: two bench.py --dump-outputs directories are
reported identical only if every array is on both sides with the same shape,
dtype and contents."""
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tools", "compare_dump.py")


def _run(a, b):
    return subprocess.run([sys.executable, TOOL, "--npy", str(a), str(b)],
                          capture_output=True, text=True, timeout=60)


def test_npy_directory_compare(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    for d in (a, b):
        d.mkdir()
        np.save(d / "x.npy", np.arange(12, dtype=np.float64).reshape(3, 4))
        np.save(d / "y.npy", np.zeros(5, dtype=np.float32))
    r = _run(a, b)
    assert r.returncode == 0 and "all 2 arrays identical" in r.stdout
    y = np.zeros(5, dtype=np.float32)
    y[3] = 1
    np.save(b / "y.npy", y)  # one value differs
    r = _run(a, b)
    assert r.returncode == 1 and "DIFFER" in r.stdout
    np.save(b / "y.npy", np.zeros(5, dtype=np.float64))  # same values, dtype
    assert _run(a, b).returncode == 1
    np.save(b / "y.npy", np.zeros(5, dtype=np.float32))
    assert _run(a, b).returncode == 0
    os.remove(b / "x.npy")  # an array missing on one side
    r = _run(a, b)
    assert r.returncode == 1 and "ONLY IN ONE" in r.stdout
    empty = tmp_path / "e"
    empty.mkdir()
    assert _run(empty, empty).returncode == 1  # nothing to compare is no pass
