"""bench.py --dump-outputs / --full plumbing.

CPU: dump_outputs() against a straightforward recomputation on synthetic
"output files" (sizes that are no multiple of the digest chunk, chunks that
straddle file boundaries, both the take-everything and the sampled branch).

GPU: one tiny plain bench run — the result line carries ms_per_step for
exactly --steps timed steps, the --full legs stay off, and the dump
describes the SSTs the last step wrote."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402

NAMES = ["job_counts", "file_meta", "file_smallest_key", "file_largest_key",
         "sst_chunk_digest", "sst_bytes_sample"]


def _fake_last(tmp_path, sizes, seed=7):
    rng = np.random.default_rng(seed)
    files = []
    for i, n in enumerate(sizes):
        p = tmp_path / ("%06d.sst" % (100 + i))
        rng.integers(0, 256, size=n, dtype=np.uint8).tofile(p)
        files.append(dict(path=str(p), file_number=100 + i, file_size=n,
                          smallest=bytes([i]) * 24, largest=bytes([i + 1]) * 20,
                          smallest_seqno=1 + i, largest_seqno=1000 + i,
                          num_entries=10 * (i + 1)))
    return dict(files=files, in_bytes=12345, out_bytes=sum(sizes),
                in_entries=77, out_entries=sum(f["num_entries"] for f in files))


def _expect_digest(cat):
    pad = (-len(cat)) % bench.DUMP_CHUNK
    rows = np.concatenate([cat, np.zeros(pad, np.uint8)]).astype(np.int64)
    rows = rows.reshape(-1, bench.DUMP_CHUNK)
    w = np.arange(bench.DUMP_CHUNK) % 16 + 1
    return np.stack([rows.sum(axis=1), (rows * w).sum(axis=1)], axis=1)


def _expect_sample(cat):
    if len(cat) <= bench.DUMP_SAMPLE:
        return cat
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(
        0, len(cat), size=bench.DUMP_SAMPLE))
    return cat[pos]


@pytest.mark.parametrize("sample_cap", [1 << 20, 5000])
def test_dump_outputs_matches_recomputation(tmp_path, monkeypatch, sample_cap):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", sample_cap)
    sizes = [10000, 4096, 1, 12289]
    last = _fake_last(tmp_path, sizes)
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), last)
    got = {n: np.load(out / (n + ".npy")) for n in NAMES}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in NAMES)
    for a in got.values():
        assert a.dtype in (np.float32, np.float64)

    cat = np.concatenate([np.fromfile(f["path"], np.uint8)
                          for f in last["files"]])
    assert np.array_equal(got["job_counts"], [12345, sum(sizes), 77, 100])
    assert np.array_equal(got["file_meta"][:, 0], sizes)
    assert np.array_equal(got["file_meta"][:, 1], [10, 20, 30, 40])
    assert np.array_equal(got["file_meta"][:, 4:], [[24, 20]] * 4)
    assert np.array_equal(got["file_smallest_key"][2, :24], [2.0] * 24)
    assert np.all(got["file_smallest_key"][:, 24:] == -1)
    assert np.array_equal(got["file_largest_key"][0, :20], [1.0] * 20)
    assert np.array_equal(got["sst_chunk_digest"], _expect_digest(cat))
    assert len(got["sst_bytes_sample"]) == min(len(cat), sample_cap)
    assert np.array_equal(got["sst_bytes_sample"], _expect_sample(cat))

    # same inputs -> same dump
    out2 = tmp_path / "dump2"
    bench.dump_outputs(str(out2), last)
    for n in NAMES:
        assert np.array_equal(got[n], np.load(out2 / (n + ".npy")))


def test_dump_outputs_key_longer_than_64(tmp_path):
    last = _fake_last(tmp_path, [100, 200])
    last["files"][1]["largest"] = bytes(range(70))
    bench.dump_outputs(str(tmp_path / "dump"), last)
    a = np.load(tmp_path / "dump" / "file_largest_key.npy")
    assert a.shape == (2, 70)
    assert np.array_equal(a[1], np.arange(70))
    assert np.all(a[0, 20:] == -1)
    assert np.load(tmp_path / "dump" / "file_smallest_key.npy").shape == (2, 64)


@pytest.mark.gpu
def test_plain_bench_run_dumps_last_step(tmp_path):
    dump = tmp_path / "dump"
    work = tmp_path / "work"
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "1", "--jobs-in-flight", "2",
         "--entries-per-run", "20000", "--workdir", str(work),
         "--dump-outputs", str(dump)],
        capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    assert r["unit"] == "MB/s" and r["higher_is_better"] is True
    in_bytes = r["config"]["input_bytes_per_job"]
    assert r["value"] == pytest.approx(
        in_bytes * 3 / (r["ms_per_step"] * 3 / 1000) / 1e6, rel=1e-3)
    # --steps sets the number of timed steps: the kernel table is reset
    # after warmup, a job decompresses its inputs in one launch and merges
    # its 8 runs pairwise in 4 + 2 + 1 launches
    assert r["kernels"]["decompress"]["launches"] == 3
    assert r["kernels"]["merge_pair"]["launches"] == 3 * 7
    # the legs that take runs of their own are behind --full
    assert r["cpu_baseline"] is None and r["hbm_resident"] is None
    assert "cpu_baseline" not in out.stderr

    got = {n: np.load(dump / (n + ".npy")) for n in NAMES}
    for a in got.values():
        assert a.dtype in (np.float32, np.float64)
    # 8 runs of distinct keys, bottommost: every entry survives
    assert got["job_counts"][0] == in_bytes
    assert got["job_counts"][2] == got["job_counts"][3] == 8 * 20000
    assert got["file_meta"][:, 1].sum() == got["job_counts"][3]
    # the dump describes the files of the last job, which are still there
    slot = work / "r0" / ("out%d" % ((3 - 1) % 2))
    cat = np.concatenate([np.fromfile(slot / f, np.uint8)
                          for f in sorted(os.listdir(slot))])
    assert len(cat) == got["file_meta"][:, 0].sum() == got["job_counts"][1]
    assert np.array_equal(got["sst_chunk_digest"], _expect_digest(cat))
    assert np.array_equal(got["sst_bytes_sample"], _expect_sample(cat))
