"""zlib output data blocks, encoded on the GPU (k_compress_zlib), by the method
of test_lz4_output_gpu.py: the worker runs with compression 2, the oracle with
none.  (a) Data region: the oracle's table builder with tests/zlib_out_spec.py
as its codec; every payload also decodes with Python's zlib.  (b) Round trip:
an uncompressed job over the worker's files (k_decompress_zlib on our own
output) against the oracle's over the raw twin."""
import os
import random
import sys
import zlib

import pytest

import oracle
import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import foreign_corpus as fc  # noqa: E402
import foreign_lz4 as fl  # noqa: E402
import zlib_out_spec as spec  # noqa: E402
from test_lz4_output_gpu import (default_runs, general_key_runs, gpu,  # noqa: E402,F401
                                 outdir, quarter_kib_values, read, write_runs)

pytestmark = pytest.mark.gpu
V, ZLIB = fc.TYPE_VALUE, 2


def check(tmp, tag, runs, data_region=True, **kw):
    """-> (the worker's result, raw size and type of the expected blocks)"""
    kw = dict(dict(bottommost_level=1), **kw)
    rg = dcw.execute(dcw.make_job(runs, outdir(tmp, tag + "_g"),
                                  compression=ZLIB, **kw))
    ro = oracle.execute(oracle.make_job(runs, outdir(tmp, tag + "_o"),
                                        compression=0, **kw))
    assert rg["out_entries"] == ro["out_entries"] > 0
    blocks, region = [], [0]
    if data_region:  # (a)
        assert len(rg["files"]) == len(ro["files"]) == 1

        def codec(raw):
            payload = spec.encode(raw)
            if payload:
                size, body = fl.unframe(payload)
                d = zlib.decompressobj(wbits=-14)
                assert d.decompress(body) == raw and d.eof and size == len(raw)
            region[0] += len(payload or raw) + 5
            blocks.append((len(raw), ZLIB if payload else 0))
            return (ZLIB, payload) if payload else None

        opts = oracle.default_table_opts(
            block_size=kw.get("block_size", 4096),
            checksum_type=kw.get("checksum_type", 4))
        want = oracle.build_sst(oracle.read_sst(read(ro["files"][0]["path"])),
                                opts, data_block_codec=codec)
        got = read(rg["files"][0]["path"])
        assert got[:region[0]] == want[:region[0]]
    # (b)
    kw2 = dict(bottommost_level=1, compression=0)
    rg2 = dcw.execute(dcw.make_job([[f["path"] for f in rg["files"]]],
                                   outdir(tmp, tag + "_g2"), **kw2))
    ro2 = oracle.execute(oracle.make_job([[f["path"] for f in ro["files"]]],
                                         outdir(tmp, tag + "_o2"), **kw2))
    assert rg2["out_entries"] == ro2["out_entries"] == rg["out_entries"]
    assert [read(f["path"]) for f in rg2["files"]] == \
        [read(f["path"]) for f in ro2["files"]]
    return rg, blocks


@pytest.mark.parametrize("checksum_type", [1, 4])
def test_default_job(tmp_path, checksum_type):
    # raw and compressed blocks; the properties name the codec ("rocksdb.comp"
    # is shared with the key before, "_options" follows the value)
    rg, blocks = check(tmp_path, "def", default_runs(tmp_path),
                       checksum_type=checksum_type)
    assert {t for _, t in blocks} == {0, ZLIB}
    assert b"ressionZlib\x13" in read(rg["files"][0]["path"])


@pytest.mark.parametrize("block_size", [16384, 16400, 40000])
def test_block_size_ladder(tmp_path, block_size):
    # blocks close within one entry below block_size: just below one window,
    # just above it, and three windows; the value of 50000 bytes makes four
    rng = random.Random(0xB5)
    kvs = [(fc.ukey(2 * i), 1 + i, V, v)
           for i, v in enumerate(quarter_kib_values(400, rng))]
    kvs.append((fc.ukey(799), 900, V, b"".join(quarter_kib_values(200, rng))[:50000]))
    newer = [(fc.ukey(3 * i), 5000 + i, V, v)
             for i, v in enumerate(quarter_kib_values(60, rng))]
    _, blocks = check(tmp_path, "bs", write_runs(tmp_path, "b", kvs, newer),
                      block_size=block_size)
    assert all(t == ZLIB for _, t in blocks)
    assert any(block_size - 300 < n <= block_size for n, _ in blocks)
    assert max(blocks)[0] > 50000


def directed_runs(tmp):
    # the directed blocks of test_zlib_output_cpu.py as values
    rng = random.Random(0x5EB)
    kvs = [(fc.ukey(10 * i), 1 + i, V, rng.randbytes(30) * 3) for i in range(80)]
    kvs += [(fc.ukey(405), 500, V, spec.boundary_block()),
            (fc.ukey(415), 501, V, spec.three_window_block())]
    return write_runs(tmp, "s", kvs)


@pytest.mark.parametrize("name,runs,kw", [
    ("directed", directed_runs, {}),
    ("general_keys", general_key_runs, {}),
    ("file_cuts", lambda tmp: default_runs(tmp, 900, 700),
     dict(data_region=False, target_file_size=16 << 10)),
], ids=["directed", "general_keys", "file_cuts"])
def test_shapes(tmp_path, name, runs, kw):
    rg, blocks = check(tmp_path, name, runs(tmp_path), **kw)
    assert (len(rg["files"]) >= 3 if name == "file_cuts" else
            sum(t == ZLIB for _, t in blocks) >= 2)


def test_pool_reuse_zlib_snappy_zlib(tmp_path):
    runs = default_runs(tmp_path)
    check(tmp_path, "p1", runs)
    rg, ro = (m.execute(m.make_job(runs, outdir(tmp_path, "p2" + m.__name__),
                                   bottommost_level=1, compression=1))
              for m in (dcw, oracle))
    assert [read(f["path"]) for f in rg["files"]] == \
        [read(f["path"]) for f in ro["files"]]
    check(tmp_path, "p3", runs)


def test_zlib_with_dzt_output_refused(tmp_path):
    out = outdir(tmp_path, "refused")
    with pytest.raises(RuntimeError, match=r"\(13\)"):
        dcw.execute(dcw.make_job(default_runs(tmp_path), out, bottommost_level=1,
                                 compression=ZLIB, output_table_factory=1))
    assert os.listdir(out) == []
