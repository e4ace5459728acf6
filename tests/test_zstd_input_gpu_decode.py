"""zstd input data blocks, decoded on the GPU (k_decompress_zstd).

Every job is a bottommost compaction.  The inputs exist twice: with data
blocks stored as type 7, varint32 + zstd frame, by libzstd or assembled by
hand (tests/foreign_zstd.py), and as raw twins of the same entries.  The GPU
reads the zstd files, the oracle the twins; the output files must be
identical byte for byte, reading them back must give the survivor list
computed in plain Python, and the kernel statistics must show
`decompress_zstd` at work on exactly the blocks the eligibility walk takes.
tests/test_zstd_decode_cpu.py runs the same frame kinds, and the malformed
streams used here, through the same decoder source on the CPU.
"""
import ctypes
import json
import os
import random
import sys

import pytest

import oracle
import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import foreign_corpus as fc  # noqa: E402
import foreign_lz4 as fl  # noqa: E402
import foreign_zstd as fz  # noqa: E402
import test_lz4_input_gpu as tl  # noqa: E402  (write, outdir, check)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    dcw.init(0)
    yield
    dcw.shutdown()


def zstd_kernel_stats():
    lib = dcw.lib()
    lib.dcw_kernel_stats_json.restype = ctypes.c_int32
    lib.dcw_kernel_stats_json.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    buf = ctypes.create_string_buffer(16384)
    lib.dcw_kernel_stats_json(buf, 16384)
    k = json.loads(buf.value.decode()).get("decompress_zstd")
    return (k["launches"], k["alg_bytes"]) if k else (0, 0)


def by_hand(raw):
    """two raw blocks in one frame, 4-byte content size"""
    h = len(raw) // 3
    return fz.hand_frame([fz.raw_block(raw[:h]), fz.raw_block(raw[h:], True)],
                         len(raw), 4)


# block index, raw block -> (frame, the walk takes it)
KINDS = {
    "level1": lambda i, raw: (fz.compress(raw, 1), True),
    "level19": lambda i, raw: (fz.compress(raw, 19), True),
    "flushed_blocks": lambda i, raw: (fz.compress(
        raw, flush_at=(len(raw) // 3, 2 * len(raw) // 3)), True),
    "by_hand": lambda i, raw: (by_hand(raw), True),
    "host_only_mixed": lambda i, raw: (
        fz.compress(raw, checksum=i % 3 == 0),
        i % 3 != 0 and len(raw) <= fz.DEC_MAX),
}


def zstd_run(kvs, kind, expect, **opts):
    """-> fl.build_pair's tuple; adds stored + decoded bytes of the blocks
    the GPU decodes to expect[0]."""
    def choose(i, raw):
        frame, eligible = KINDS[kind](i, raw)
        if eligible:
            expect[0] += len(fz.frame_block(frame, len(raw))) + len(raw)
        return fz.ZSTD, frame
    return fl.build_pair(kvs, choose, **dict(dict(block_size=4096), **opts))


def check(tmp, job, expect_bytes, **kw):
    """tl.check (GPU on the ssts against the oracle on the raw twins, and the
    plain-Python survivor list), and the zstd kernel's account."""
    dcw.lib().dcw_kernel_stats_reset()
    tl.check(tmp, job, **kw)
    launches, alg_bytes = zstd_kernel_stats()
    assert (launches > 0, alg_bytes) == (expect_bytes > 0, expect_bytes)


def two_runs(seed, big=False):
    rng = random.Random(seed)
    kv0, kv1 = fc.two_runs(700, 500, rng)
    if big:  # one 16 KiB block: beyond the decoder's staging, host-only
        kv0 = sorted(kv0 + [(fc.ukey(3), 70000, fc.TYPE_VALUE,
                             fz._record_text(16384, rng))])
    return kv0, kv1


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_frame_kinds(tmp_path, kind):
    expect = [0]
    kv0, kv1 = two_runs(0x70 + sorted(KINDS).index(kind),
                        big=kind == "host_only_mixed")
    job = [zstd_run(kv0, kind, expect),
           zstd_run(kv1, "level1" if kind != "level1" else "level19", expect)]
    check(tmp_path, job, expect[0])


@pytest.mark.parametrize("mode", ["staged", "beside_lz4_and_snappy", "host_env"])
def test_paths_around_the_kernel(tmp_path, monkeypatch, mode):
    expect = [0]
    kv0, kv1 = two_runs(0x7A)
    job = [zstd_run(kv0, "level1", expect)]
    if mode == "beside_lz4_and_snappy":
        entries = [(oracle.make_ikey(k, s + 200000, t), v)
                   for k, s, t, v in two_runs(0x7B)[0]]
        kv2 = [(k, s + 200000, t, v) for k, s, t, v in two_runs(0x7B)[0]]
        snap = oracle.build_sst(entries, oracle.default_table_opts(compression=1))
        job += [fl.build_pair(kv1, lambda i, raw: (fl.LZ4, fl.best(raw)),
                              block_size=4096), (kv2, snap, snap, [])]
        check(tmp_path, job, expect[0], compression=1)
        return
    job.append(zstd_run(kv1, "flushed_blocks", expect))
    if mode == "host_env":  # every block down the host path, same files
        monkeypatch.setenv("DCW_ZSTD_HOST", "1")
        expect[0] = 0
    check(tmp_path, job, expect[0], staged=mode == "staged")


# refused by libzstd, accepted by the eligibility walk, refused sanitizer-clean
# by tools/zstd_host (tests/test_zstd_decode_cpu.py runs all of fz.mutations())
MALFORMED = ["records_l3.flip10@10", "skewed_deep_tree.flip13@1979",
             "three_blocks.flip25@358", "few_symbols.flip17@24",
             "count_65.flip18@90"]


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    d = tmp_path_factory.mktemp("good")
    job = [zstd_run(kv, "level1", [0]) for kv in two_runs(0x7C)]
    runs = [[tl.write(d, "in%d.sst" % i, r[1])] for i, r in enumerate(job)]
    twins = [[tl.write(d, "twin%d.sst" % i, r[2])] for i, r in enumerate(job)]
    kw = dict(compression=0, bottommost_level=1)
    return runs, twins, kw


@pytest.mark.parametrize("name", MALFORMED)
def test_malformed_frame_refused(tmp_path, good, name):
    """A bounds decision, not a fault: refused with no output, and the worker
    runs a good job right after."""
    (payload,) = [p for n, p, want in fz.mutations()
                  if n == name and want is None]
    rng = random.Random(0xE7)
    entries = [(oracle.make_ikey(fc.ukey(i), 1 + i, fc.TYPE_VALUE), v)
               for i, v in enumerate(fc.mixed_values(150, rng))]
    count = [0]

    def codec(raw):
        count[0] += 1
        if count[0] == 2:
            return fz.ZSTD, payload
        return fz.ZSTD, fz.frame_block(fz.compress(raw), len(raw))

    p = tl.write(tmp_path, "bad.sst", oracle.build_sst(
        entries, oracle.default_table_opts(block_size=4096),
        data_block_codec=codec))
    assert count[0] >= 3
    out = tl.outdir(tmp_path, "bad_out")
    with pytest.raises(RuntimeError):
        dcw.execute(dcw.make_job([[p]], out, bottommost_level=1))
    assert os.listdir(out) == []
    runs, twins, kw = good
    tl.assert_identical(
        dcw.execute(dcw.make_job(runs, tl.outdir(tmp_path, "good_out"), **kw)),
        oracle.execute(oracle.make_job(twins, tl.outdir(tmp_path, "orc"), **kw)))
