"""Level-below and grandparent boundaries of any key length on the GPU
worker: one test per job of tests/bounds_corpus.py.

Every job is checked twice, both exactly, as in
tests/test_foreign_input_gpu.py: the output files and their
smallest/largest/seqno metadata are bit-identical to the oracle's, and
reading the files back gives the survivor list computed in plain Python
where the model applies.  tests/test_bounds_cpu.py asserts on the CPU that
each job of the groups bounds_corpus.SEPARATING gives another result when
boundaries are compared as zero-padded 16-byte words, so a worker that
compares that way fails here.

All jobs run on one worker; the last test runs a default job on it, to show
that the boundary tables of one job do not leak into the next.
"""
import os
import sys

import pytest

import oracle
import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds_corpus as bc  # noqa: E402
from test_worker_gpu import gen_runs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    dcw.init(0)
    yield
    dcw.shutdown()


def assert_identical(rg, ro):
    assert rg["out_entries"] == ro["out_entries"]
    assert [f["largest"] for f in rg["files"]] == \
        [f["largest"] for f in ro["files"]]
    assert len(rg["files"]) == len(ro["files"])
    for fg, fo in zip(rg["files"], ro["files"]):
        assert fg["file_number"] == fo["file_number"]
        with open(fg["path"], "rb") as a, open(fo["path"], "rb") as b:
            da, db = a.read(), b.read()
        assert da == db, "GPU SST %s differs from oracle (sizes %d vs %d)" % (
            fg["path"], len(da), len(db))
        for field in ("smallest", "largest", "smallest_seqno", "largest_seqno"):
            assert fg[field] == fo[field], field


def read_back(files):
    got = []
    for f in files:
        with open(f["path"], "rb") as fh:
            got += oracle.read_sst(fh.read())
    return got


def run_and_check(tmp_path, job):
    runs = job.write_inputs(tmp_path)
    out_o = tmp_path / "orc"
    out_g = tmp_path / "gpu"
    out_o.mkdir()
    out_g.mkdir()
    ro = oracle.execute(oracle.make_job(runs, str(out_o), **job.kw()))
    rg = dcw.execute(dcw.make_job(runs, str(out_g), **job.kw()))
    got = read_back(rg["files"])
    if job.model:
        # first, so that a failure names the keys
        kept = {k for k, v in got}
        want = {k for k, v in job.expected}
        assert kept == want, "kept but not expected %r, dropped but expected %r" % (
            sorted(kept - want), sorted(want - kept))
        assert got == job.expected
    assert_identical(rg, ro)
    assert got == read_back(ro["files"])


@pytest.mark.parametrize("name", bc.names(bc.level_below_jobs()))
def test_level_below(tmp_path, name):
    run_and_check(tmp_path, bc.by_name(name))


@pytest.mark.parametrize("name", bc.names(bc.grandparent_jobs()))
def test_grandparent(tmp_path, name):
    job = bc.by_name(name)
    run_and_check(tmp_path, job)


def test_default_job_after_boundary_jobs(tmp_path):
    # what the boundary jobs left in the worker's device tables (lengths,
    # general-mode boundary bytes) must not reach a job without boundaries
    job = bc.by_name("general_bound_60")
    d = tmp_path / "before"
    d.mkdir()
    run_and_check(d, job)
    runs = gen_runs(tmp_path, 2, 1000)
    out_o = tmp_path / "orc"
    out_g = tmp_path / "gpu"
    out_o.mkdir()
    out_g.mkdir()
    kw = dict(target_file_size=64 << 20)
    rg = dcw.execute(dcw.make_job(runs, str(out_g), **kw))
    ro = oracle.execute(oracle.make_job(runs, str(out_o), **kw))
    assert_identical(rg, ro)
