"""Input files with a preset dictionary ("rocksdb.compression_dict"), decoded
on the GPU with it.  As tests/test_lz4_input_gpu.py: the GPU reads files coded
against a dictionary by foreign encoders (tests/foreign_dict.py), the oracle
their raw twins; outputs must be identical byte for byte.
tests/test_dict_input_cpu.py runs the same blocks and refusals on the CPU."""
import os
import random
import sys

import pytest

import oracle
import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import foreign_dict as fd  # noqa: E402
import foreign_lz4 as fl  # noqa: E402
import foreign_zstd as fz  # noqa: E402
import test_lz4_input_gpu as tl  # noqa: E402  (write, outdir, check)
from test_lz4_input_gpu import gpu  # noqa: E402,F401  (init / shutdown fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", fd.ZSTD_CASES)
def test_zstd(tmp_path, name):
    tl.check(tmp_path, fd.zstd_job(name))


@pytest.mark.parametrize("name,btype", [(n, fl.LZ4) for n in sorted(fd.LZ4_CASES)] +
                         [("dict_4k", fl.LZ4HC)])
def test_lz4(tmp_path, name, btype):
    tl.check(tmp_path, fd.lz4_job(name, btype))


@pytest.mark.parametrize("check_kw,env", [
    (dict(), {"DCW_ZSTD_HOST": "1"}), (dict(staged=True), {}), (dict(compression=1), {})],
    ids=["zstd_host_env", "staged", "snappy_output"])
def test_other_paths(tmp_path, monkeypatch, check_kw, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tl.check(tmp_path, fd.zstd_job("trained_4k"), **check_kw)


def test_mixed_job(tmp_path):
    """two dictionaries, zstd without one, a dictionary file of raw/zstd/snappy blocks"""
    rng = random.Random(0x3D)
    d1, d2 = fd.trained(4096), fd.trained(16384)
    a = fd.dict_run(fd.text_kvs([900] * 150, rng), d1, fd.zstd_choose(d1), block_size=4096)
    b = fd.dict_run(fd.text_kvs([700] * 150, rng, base=1), d2,
                    fd.zstd_choose(d2, level=19), block_size=8192)
    kv = [(k, 7000 + s, t, v) for k, s, t, v in fd.text_kvs([500] * 100, rng, base=40)]
    c = fl.build_pair(kv, lambda i, raw: (fz.ZSTD, fz.compress(raw)), block_size=4096)
    kv = [(k, 9000 + s, t, v) for k, s, t, v in fd.text_kvs([1500] * 90, rng, base=100)]

    def choose(i, raw):
        if i % 3 == 2:  # build_pair puts the varint32 preamble back in front
            return 1, oracle.snappy_compress(raw)[len(fl.put_varint32(len(raw))):]
        return (fz.ZSTD, fd.compress(raw, d1)) if i % 3 else None

    tl.check(tmp_path, [a, b, c, fd.dict_run(kv, d1, choose, block_size=2048)])


@pytest.mark.parametrize("name", sorted(fd.refusals()))
def test_refused(tmp_path, name):
    """A bounds decision, not a fault: no output, and a good job right after.
    tools/*_dict_host refused each sanitizer-clean; libzstd refuses the zstd ones."""
    dic, btype, payload, _ = fd.refusals()[name]
    count = [0]

    def codec(raw):
        count[0] += 1
        return (btype, payload) if count[0] == 2 else None

    entries = [(oracle.make_ikey(k, s, t), v)
               for k, s, t, v in fd.text_kvs([1500] * 12, random.Random(0xBAD))]
    p = tl.write(tmp_path, "bad.sst", fd.add_dict_block(oracle.build_sst(
        entries, oracle.default_table_opts(block_size=4096), data_block_codec=codec), dic))
    assert count[0] >= 3
    out = tl.outdir(tmp_path, "bad_out")
    with pytest.raises(RuntimeError):
        dcw.execute(dcw.make_job([[p]], out, bottommost_level=1))
    assert os.listdir(out) == []
    tl.check(tmp_path, fd.lz4_job("dict_4k"))
