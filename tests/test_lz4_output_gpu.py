"""LZ4 and LZ4HC output data blocks, encoded on the GPU (k_compress_lz4).
The worker runs with compression 4 or 5, the oracle, which writes no LZ4,
with none (the raw twin).  (a) Data region, single-file jobs: the twin's
entries through the oracle's table builder with tests/lz4_out_spec.py as its
codec give every payload, type byte and checksum.  (b) Round trip: a second,
uncompressed job over the worker's LZ4 files must give, whole files, what
the oracle gives over the twin's files."""
import os
import random
import sys

import pytest

import oracle
import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import big_block_corpus as bb  # noqa: E402
import foreign_corpus as fc  # noqa: E402
import lz4_out_spec as spec  # noqa: E402

pytestmark = pytest.mark.gpu
V = fc.TYPE_VALUE


@pytest.fixture(scope="module", autouse=True)
def gpu():
    dcw.init(0)
    yield
    dcw.shutdown()


def read(path):
    with open(path, "rb") as f:
        return f.read()


def outdir(tmp, name):
    os.makedirs(os.path.join(str(tmp), name))
    return os.path.join(str(tmp), name)


def check(tmp, tag, runs, ctype, data_region=True, **kw):
    """-> (the worker's result, raw size and type of the expected blocks)"""
    kw = dict(dict(bottommost_level=1), **kw)
    rg = dcw.execute(dcw.make_job(runs, outdir(tmp, tag + "_g"),
                                  compression=ctype, **kw))
    ro = oracle.execute(oracle.make_job(runs, outdir(tmp, tag + "_o"),
                                        compression=0, **kw))
    assert rg["out_entries"] == ro["out_entries"] > 0
    blocks, region = [], [0]
    if data_region:  # (a)
        assert len(rg["files"]) == len(ro["files"]) == 1

        def codec(raw):
            payload = spec.encode(raw)
            region[0] += len(payload or raw) + 5
            blocks.append((len(raw), ctype if payload else 0))
            return (ctype, payload) if payload else None

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


def write_runs(tmp, tag, *runs_kvs):
    return [[bb.write_run(tmp, "%s%d.sst" % (tag, i), kvs)]
            for i, kvs in enumerate(runs_kvs)]


def default_runs(tmp, n0=300, n1=200):
    # mixed values, and a stretch of random ones that fills whole blocks
    rng = random.Random(0x0D4)
    kv0, kv1 = fc.two_runs(n0, n1, rng)
    kv0[100:160] = [(k, s, t, rng.randbytes(400)) for k, s, t, _ in kv0[100:160]]
    return write_runs(tmp, "d", kv0, kv1)


@pytest.mark.parametrize("checksum_type", [1, 4])
@pytest.mark.parametrize("ctype,name", [(4, b"LZ4"), (5, b"LZ4HC")])
def test_default_job(tmp_path, ctype, name, checksum_type):
    # raw and compressed blocks; the properties name the codec ("rocksdb.comp"
    # is shared with the key before, "_options" follows the value)
    rg, blocks = check(tmp_path, "def", default_runs(tmp_path), ctype,
                       checksum_type=checksum_type)
    assert {t for _, t in blocks} == {0, ctype}
    assert b"ression" + name + b"\x13" in read(rg["files"][0]["path"])


def quarter_kib_values(n, rng):  # half random, half words: accepted
    words = [rng.randbytes(rng.randint(3, 9)) for _ in range(30)]
    return [rng.randbytes(120) + b" ".join(rng.choices(words, k=30))[:130]
            for _ in range(n)]


@pytest.mark.parametrize("block_size", [16384, 16400, 65536, 65836])
def test_block_size_ladder(tmp_path, block_size):
    # blocks close within one entry below block_size: just below one window
    # and just above it; the value of 200000 bytes makes four windows
    rng = random.Random(0xB5)
    kvs = [(fc.ukey(2 * i), 1 + i, V, v)
           for i, v in enumerate(quarter_kib_values(600, rng))]
    kvs.append((fc.ukey(1199), 900, V,
                b"".join(quarter_kib_values(800, rng))[:200000]))
    newer = [(fc.ukey(3 * i), 5000 + i, V, v)
             for i, v in enumerate(quarter_kib_values(100, rng))]
    _, blocks = check(tmp_path, "bs", write_runs(tmp_path, "b", kvs, newer), 4,
                      block_size=block_size)
    assert all(t == 4 for _, t in blocks)
    assert any(block_size - 300 < n <= block_size for n, _ in blocks)
    assert max(blocks)[0] > 200000


def seam_runs(tmp):
    # the directed block of test_lz4_output_cpu.py as a value
    rng = random.Random(0x5EB)
    kvs = [(fc.ukey(10 * i), 1 + i, V, rng.randbytes(30) * 3)
           for i in range(80)]
    return write_runs(tmp, "s", kvs + [(fc.ukey(405), 500, V, spec.seam_block())])


def general_key_runs(tmp):
    rng = random.Random(0x6E5)
    keys = sorted({rng.randbytes(rng.choice([6, 10, 16, 24, 33, 48]))
                   for _ in range(400)})
    kvs = [(k, 1 + i, V, v)
           for i, (k, v) in enumerate(zip(keys, fc.mixed_values(400, rng)))]
    return write_runs(tmp, "g", kvs[0::2], kvs[1::2])


@pytest.mark.parametrize("name,runs,ctype,kw", [
    ("seam", seam_runs, 4, {}),
    ("general_keys", general_key_runs, 5, {}),
    ("file_cuts", lambda tmp: default_runs(tmp, 900, 700), 4,
     dict(data_region=False, target_file_size=16 << 10)),
], ids=["seam", "general_keys", "file_cuts"])
def test_shapes(tmp_path, name, runs, ctype, kw):
    rg, blocks = check(tmp_path, name, runs(tmp_path), ctype, **kw)
    assert (len(rg["files"]) >= 3 if name == "file_cuts" else
            sum(t == ctype for _, t in blocks) >= 2)


def test_pool_reuse_lz4_snappy_lz4(tmp_path):
    runs = default_runs(tmp_path)
    check(tmp_path, "p1", runs, 4)
    rg, ro = (m.execute(m.make_job(runs, outdir(tmp_path, "p2" + m.__name__),
                                   bottommost_level=1, compression=1))
              for m in (dcw, oracle))
    assert [read(f["path"]) for f in rg["files"]] == \
        [read(f["path"]) for f in ro["files"]]
    check(tmp_path, "p3", runs, 5)


@pytest.mark.parametrize("kw", [dict(compression=7),
                                dict(compression=4, output_table_factory=1)],
                         ids=["zstd", "lz4_dzt"])
def test_still_refused(tmp_path, kw):
    out = outdir(tmp_path, "refused")
    with pytest.raises(RuntimeError, match=r"\(13\)"):
        dcw.execute(dcw.make_job(default_runs(tmp_path), out,
                                 bottommost_level=1, **kw))
    assert os.listdir(out) == []
