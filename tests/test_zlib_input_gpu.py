"""zlib input data blocks, decoded on the GPU (k_decompress_zlib).  The inputs
exist twice (tests/foreign_zlib.py): data blocks stored as type 2 by Python's
zlib, and raw twins of the same entries.  The GPU reads the zlib files, the
oracle the twins; the output files must be identical byte for byte."""
import os
import sys

import pytest

import oracle
import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dzt_foreign as zf  # noqa: E402
import foreign_dict as fd  # noqa: E402
import foreign_lz4 as fl  # noqa: E402
import foreign_zlib as fz  # noqa: E402
import test_lz4_input_gpu as tl  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    dcw.init(0)
    yield
    dcw.shutdown()


JOBS = dict({p: lambda p=p: fz.policy_job(p) for p in fz.POLICIES},
            fibonacci=fz.fibonacci_job, staging_edge=fz.edge_job,
            block_64k=lambda: fz.large_job("block_64k"),
            value_200k=lambda: fz.large_job("value_200k"),
            zlib_raw_lz4_snappy_zlib_index=fz.mixed_job)


@pytest.mark.parametrize("name", sorted(JOBS))
def test_job(tmp_path, name):
    tl.check(tmp_path, JOBS[name]())


@pytest.mark.parametrize("kw", [dict(staged=True), dict(compression=1)],
                         ids=["staged", "snappy_output"])
def test_staging_and_output(tmp_path, kw):
    tl.check(tmp_path, fz.mixed_job(), **kw)


def test_next_to_dzt_input(tmp_path):
    """a zlib run over a DcwZipTable run (16-byte user keys)"""
    es = [(oracle.make_ikey(zf.ukey(2 * i, 16), 1000 + i, 1), b"older-%d" % i * 9)
          for i in range(600)]
    files = zf.oracle_dzt(tmp_path, "z", es)
    twin = [tl.write(tmp_path, "ztwin%d.sst" % i, zf.twin_sst(p)) for i, p in enumerate(files)]
    newer = [(oracle.make_ikey(zf.ukey(3 * i, 16), 900000 + i, int(i % 4 != 0)),
              b"" if i % 4 == 0 else b"newer-%d" % i * 11) for i in range(400)]
    to = oracle.default_table_opts(block_size=4096)
    zl = tl.write(tmp_path, "zlib.sst", oracle.build_sst(
        newer, to, data_block_codec=lambda raw: (fz.ZLIB, fl.frame(fz.deflate(raw), len(raw)))))
    raw = tl.write(tmp_path, "raw.sst", oracle.build_sst(newer, to))
    kw = dict(compression=1, bottommost_level=1)
    ro = oracle.execute(oracle.make_job([[raw], twin], tl.outdir(tmp_path, "orc"), **kw))
    rg = dcw.execute(dcw.make_job([[zl], files], tl.outdir(tmp_path, "gpu"), **kw))
    tl.assert_identical(rg, ro)
    assert rg["out_entries"] == 600 + 400 - 400 // 4 - 200 > 0


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    d = tmp_path_factory.mktemp("good")
    job = fz.policy_job("dynamic_6")
    runs = [[tl.write(d, "in%d.sst" % i, r[1])] for i, r in enumerate(job)]
    twins = [[tl.write(d, "twin%d.sst" % i, r[2])] for i, r in enumerate(job)]
    kw = dict(compression=0, bottommost_level=1)
    return runs, kw, oracle.execute(oracle.make_job(twins, tl.outdir(d, "orc"), **kw))


def refused(tmp_path, good, sst, match=None):
    """refused with no output, and the worker runs a good job right after"""
    p = tl.write(tmp_path, "bad.sst", sst)
    out = tl.outdir(tmp_path, "bad_out")
    with pytest.raises(RuntimeError, match=match):
        dcw.execute(dcw.make_job([[p]], out, bottommost_level=1))
    assert os.listdir(out) == []
    runs, kw, ro = good
    tl.assert_identical(dcw.execute(dcw.make_job(runs, tl.outdir(tmp_path, "good_out"), **kw)), ro)


@pytest.mark.parametrize("name", fz.MALFORMED_NAMES)
def test_malformed_stream_refused(tmp_path, good, name):
    """A bounds decision, not a fault."""
    stream, size = fz.malformed(fz.word_text(3000, fz.random.Random(2)))[name]
    assert fz.verdict(stream, size) is None
    refused(tmp_path, good, fz.one_block_input(stream, size))


def test_trailing_bytes_accepted(tmp_path):
    """bytes behind the final block are no error, as for Zlib_Uncompress"""
    job = [fl.build_pair(r[0], lambda i, raw: (fz.ZLIB, fz.deflate(raw) + fz.TRAILING),
                         block_size=4096) for r in fz.policy_job("dynamic_6")]
    tl.check(tmp_path, job)


def test_dictionary_file_refused_by_name(tmp_path, good):
    sst = fd.add_dict_block(fz.policy_job("dynamic_6")[0][1], b"some dictionary bytes" * 20)
    refused(tmp_path, good, sst, match="zlib blocks with a preset dictionary")
