"""LZ4 and LZ4HC input data blocks, decoded on the GPU (k_decompress_lz4).

Every job is a bottommost compaction of two runs.  The inputs exist twice
(tests/foreign_lz4.py): with data blocks stored as type 4 or 5, varint32 +
LZ4 stream, by encoders that are not the project's, and as raw twins of the
same entries.  The GPU reads the LZ4 files, the oracle reads the twins; the
output files must be identical byte for byte, and reading them back must give
the survivor list computed in plain Python.  tests/test_lz4_input_cpu.py runs
every stream of these files through the same decoder source on the CPU.
"""
import os
import sys

import pytest

import oracle
import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dzt_foreign as zf  # noqa: E402
import foreign_corpus as fc  # noqa: E402
import foreign_lz4 as fl  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    dcw.init(0)
    yield
    dcw.shutdown()


def write(tmp, name, data):
    p = os.path.join(str(tmp), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def outdir(tmp, name):
    d = os.path.join(str(tmp), name)
    os.makedirs(d)
    return d


def assert_identical(rg, ro):
    assert rg["out_entries"] == ro["out_entries"]
    assert len(rg["files"]) == len(ro["files"])
    for fg, fo in zip(rg["files"], ro["files"]):
        with open(fg["path"], "rb") as a, open(fo["path"], "rb") as b:
            assert a.read() == b.read(), fg["path"] + " differs from oracle"
        for field in ("file_number", "smallest", "largest", "smallest_seqno",
                      "largest_seqno"):
            assert fg[field] == fo[field], field


def check(tmp, job, staged=False, **kw):
    """job: runs of (kvs, sst, twin, stored blocks), as fl.build_pair makes
    them.  GPU on the ssts against the oracle on the twins."""
    kw = dict(dict(compression=0, bottommost_level=1), **kw)
    runs = [[write(tmp, "in%d.sst" % i, r[1])] for i, r in enumerate(job)]
    twins = [[write(tmp, "twin%d.sst" % i, r[2])] for i, r in enumerate(job)]
    ro = oracle.execute(oracle.make_job(twins, outdir(tmp, "orc"), **kw))
    jd = dcw.make_job(runs, outdir(tmp, "gpu"), **kw)
    if staged:
        jd.staged_handle = dcw.stage_inputs(jd)
    rg = dcw.execute(jd)
    if staged:
        dcw.release_staged(jd.staged_handle)
    assert_identical(rg, ro)
    got = []
    for f in rg["files"]:
        with open(f["path"], "rb") as fh:
            got += oracle.read_sst(fh.read())
    assert got == fc.survivors([r[0] for r in job])
    assert rg["out_entries"] == len(got) > 0


@pytest.mark.parametrize("policy,btype", [
    (p, fl.LZ4) for p in sorted(fl.POLICIES)] + [("all_literal", fl.LZ4HC)])
def test_encoder_policy(tmp_path, policy, btype):
    if fl.POLICIES[policy](b"probe") is None:
        pytest.skip("liblz4 is not installed")
    check(tmp_path, fl.policy_job(policy, btype))


JOBS = {"directed": fl.directed_job, "dec_max": fl.decmax_job,
        "block_128k": fl.big_job, "raw_lz4_snappy": fl.alternating_job}


@pytest.mark.parametrize("name", sorted(JOBS))
def test_shapes(tmp_path, name):
    check(tmp_path, JOBS[name]())


@pytest.mark.parametrize("kw", [dict(compression=1), dict(staged=True)],
                         ids=["snappy_output", "staged"])
def test_output_and_staging(tmp_path, kw):
    check(tmp_path, fl.alternating_job(), **kw)


@pytest.mark.parametrize("other", ["dzt", "zstd"])
def test_next_to_other_input_kinds(tmp_path, other):
    """An LZ4 run over a DcwZipTable run / a zstd run (16-byte user keys)."""
    es = [(oracle.make_ikey(zf.ukey(2 * i, 16), 1000 + i, 1),
           b"older-%d" % i * 9) for i in range(1200)]
    if other == "dzt":
        files = zf.oracle_dzt(tmp_path, "z", es)
        twin = [write(tmp_path, "ztwin%d.sst" % i, zf.twin_sst(p))
                for i, p in enumerate(files)]
    else:
        files = twin = [write(tmp_path, "zstd.sst", oracle.build_sst(
            es, oracle.default_table_opts(compression=7)))]
    newer = [(oracle.make_ikey(zf.ukey(3 * i, 16), 900000 + i, int(i % 4 != 0)),
              b"" if i % 4 == 0 else b"newer-%d" % i * 11) for i in range(800)]
    to = oracle.default_table_opts(block_size=4096)
    lz4 = write(tmp_path, "lz4.sst", oracle.build_sst(
        newer, to, data_block_codec=lambda raw: (
            fl.LZ4, fl.frame(fl.best(raw), len(raw)))))
    raw = write(tmp_path, "raw.sst", oracle.build_sst(newer, to))
    kw = dict(compression=1, bottommost_level=1)
    ro = oracle.execute(oracle.make_job([[raw], twin],
                                        outdir(tmp_path, "orc"), **kw))
    rg = dcw.execute(dcw.make_job([[lz4], files],
                                  outdir(tmp_path, "gpu"), **kw))
    assert_identical(rg, ro)
    assert rg["out_entries"] == 1200 + 800 - 800 // 4 - 400 > 0


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    d = tmp_path_factory.mktemp("good")
    job = fl.alternating_job()
    runs = [[write(d, "in%d.sst" % i, r[1])] for i, r in enumerate(job)]
    twins = [[write(d, "twin%d.sst" % i, r[2])] for i, r in enumerate(job)]
    kw = dict(compression=0, bottommost_level=1)
    return runs, kw, oracle.execute(
        oracle.make_job(twins, outdir(d, "orc"), **kw))


@pytest.mark.parametrize("name", fl.MALFORMED_NAMES)
def test_malformed_stream_refused(tmp_path, good, name):
    """A bounds decision, not a fault: refused with no output, and the worker
    runs a good job right after."""
    p = write(tmp_path, "bad.sst", fl.malformed_input(name))
    out = outdir(tmp_path, "bad_out")
    with pytest.raises(RuntimeError):
        dcw.execute(dcw.make_job([[p]], out, bottommost_level=1))
    assert os.listdir(out) == []
    runs, kw, ro = good
    assert_identical(dcw.execute(
        dcw.make_job(runs, outdir(tmp_path, "good_out"), **kw)), ro)
