"""Snappy output with data blocks over 16 KiB (k_compress_large): one large
value, or a large block_size.  Every comparison is whole output files byte
for byte against the oracle, plus smallest, largest and out_entries.  The
values and the ladder are those of tests/big_block_corpus.py, which the CPU
test runs through the same encoder source under sanitizers."""
import json
import os
import random
import subprocess
import sys

import pytest

import oracle
import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import big_block_corpus as bb  # noqa: E402

pytestmark = pytest.mark.gpu

V, D = bb.TYPE_VALUE, bb.TYPE_DELETION
# runs a manifest of jobs on the worker in a fresh process
RUNNER = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      "foreign_variant_runner.py")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    dcw.init(0)
    yield
    dcw.shutdown()


def run_both(tmp_path, tag, runs, **kw):
    og = tmp_path / (tag + "_g")
    oo = tmp_path / (tag + "_o")
    og.mkdir()
    oo.mkdir()
    rg = dcw.execute(dcw.make_job(runs, str(og), **kw))
    ro = oracle.execute(oracle.make_job(runs, str(oo), **kw))
    assert rg["out_entries"] == ro["out_entries"]
    assert len(rg["files"]) == len(ro["files"])
    for fg, fo in zip(rg["files"], ro["files"]):
        with open(fg["path"], "rb") as a, open(fo["path"], "rb") as b:
            assert a.read() == b.read(), fg["path"]
        assert fg["smallest"] == fo["smallest"]
        assert fg["largest"] == fo["largest"]
        assert fg["num_entries"] == fo["num_entries"]
    return rg, ro


def oracle_blocks(res):
    out = []
    for f in res["files"]:
        with open(f["path"], "rb") as fh:
            out += bb.data_blocks(fh.read())
    return out


def small_value(rng):
    # 100 bytes, half of them a repeat: small blocks that still compress
    return rng.randbytes(50) * 2


def test_size_ladder(tmp_path):
    """One entry per block (block_size 64), periodic values sized so that
    data blocks of exactly the ladder sizes occur, all stored compressed."""
    rng = random.Random(0x1AD)
    old, new = [], []
    for i in range(120):
        old.append((bb.k16(10 * i), 1 + i, V, small_value(rng)))
    for j, size in enumerate(bb.LADDER):
        vlen = bb.value_len_for_block(size)
        kv = (bb.k16(10 * (7 + 13 * j) + 5), 500 + j, V,
              bb.periodic(vlen, size))
        (old if j % 2 else new).append(kv)
    for i in range(0, 120, 9):  # the newer run rewrites and deletes
        new.append((bb.k16(10 * i), 1000 + i, D if i % 2 else V,
                    b"" if i % 2 else small_value(rng)))
    runs = [[bb.write_run(tmp_path, "old.sst", old)],
            [bb.write_run(tmp_path, "new.sst", new)]]
    _, ro = run_both(tmp_path, "ladder", runs, bottommost_level=1,
                     compression=1, block_size=64)
    compressed = {unc for _, _, btype, unc in oracle_blocks(ro) if btype == 1}
    raw = {unc for _, _, btype, unc in oracle_blocks(ro) if btype == 0}
    for size in bb.LADDER:
        assert size in compressed and size not in raw, size


def shapes_runs(tmp_path):
    """The four large value shapes among 100-byte values, default
    block_size: a large entry is admitted whole into the block that the
    small entries before it left open."""
    rng = random.Random(0x5AE)
    old = [(bb.k16(10 * i), 1 + i, V, small_value(rng)) for i in range(300)]
    new = []
    for j, (name, val) in enumerate(sorted(bb.shapes().items())):
        kv = (bb.k16(10 * (37 + 61 * j) + 5), 2000 + j, V, val)
        (old if j % 2 else new).append(kv)
    for i in range(3, 300, 11):
        new.append((bb.k16(10 * i), 3000 + i, D if i % 2 else V,
                    b"" if i % 2 else small_value(rng)))
    return [[bb.write_run(tmp_path, "s_old.sst", old)],
            [bb.write_run(tmp_path, "s_new.sst", new)]]


@pytest.mark.parametrize("checksum_type", [1, 4])
def test_value_shapes(tmp_path, checksum_type):
    runs = shapes_runs(tmp_path)
    _, ro = run_both(tmp_path, "shapes", runs, bottommost_level=1,
                     compression=1, checksum_type=checksum_type)
    blocks = oracle_blocks(ro)
    big = {len(v): name for name, v in bb.shapes().items()}
    seen = {}
    for _, sz, btype, unc in blocks:
        for vlen, name in big.items():
            if vlen < unc < vlen + 4096 + 200:
                # more than the value alone: small entries came before it
                assert unc > vlen + 37 + 100, name
                seen[name] = btype
    assert seen == {"periodic70k": 1, "far201k": 1, "random20k": 0,
                    "random20k_twice": 1}


def kib_values_runs(tmp_path, n_old, n_new, seed):
    """About 1 KiB per value, half random and half of one shared period, two
    runs with overlapping keys and tombstones.  The period is the same in
    every value: the codec's table keeps the FIRST position of a hash slot,
    so in a 64 KiB block only what repeats the block's first few KiB
    compresses, at offsets that grow to the block's size."""
    rng = random.Random(seed)
    pat = bb.periodic(600, 0x23, 23)

    def val():
        ln = rng.randint(900, 1150)
        return rng.randbytes(ln // 2) + pat[:ln - ln // 2]
    old = [(bb.k16(2 * i), 1 + i, V, val()) for i in range(n_old)]
    new = []
    for i in range(n_new):
        dele = rng.random() < 0.25
        new.append((bb.k16(3 * i), 100000 + i, D if dele else V,
                    b"" if dele else val()))
    return [[bb.write_run(tmp_path, "k_old.sst", old)],
            [bb.write_run(tmp_path, "k_new.sst", new)]]


@pytest.mark.parametrize("block_size,bottom,target", [
    (65536, 1, 64 << 20),
    (32768, 0, 64 << 20),
    (65536, 0, 96 << 10),  # several files: the cutter sees large blocks
])
def test_large_block_size(tmp_path, block_size, bottom, target):
    runs = kib_values_runs(tmp_path, 420, 260, block_size + bottom)
    rg, ro = run_both(tmp_path, "bs", runs, bottommost_level=bottom,
                      compression=1, block_size=block_size,
                      target_file_size=target)
    blocks = oracle_blocks(ro)
    large = [b for b in blocks if b[3] > bb.SNAP_MAX_UNC]
    assert len(large) >= len(blocks) - len(ro["files"])  # all but file tails
    assert all(btype == 1 for _, _, btype, _ in large)
    if target < (1 << 20):
        assert len(ro["files"]) >= 3


def test_round_trip_through_own_decoders(tmp_path):
    """A large-block output is the input of a second job: the worker's own
    decoders read the new streams (4-byte offsets, long literals)."""
    rg, _ = run_both(tmp_path, "rt1", shapes_runs(tmp_path),
                     bottommost_level=1, compression=1)
    rng = random.Random(0x271)
    newer = [(bb.k16(10 * i), 9000 + i, D if i % 3 == 0 else V,
              b"" if i % 3 == 0 else small_value(rng))
             for i in range(0, 300, 7)]
    far_key = bb.k16(10 * 37 + 5)  # "far201k" sorts first among the shapes
    newer.append((bb.k16(10 * (37 + 61) + 5), 9500, D, b""))
    newer.append((bb.k16(10 * 299 + 7), 9501, V, bb.shapes()["periodic70k"]))
    runs = [[bb.write_run(tmp_path, "rt_new.sst", newer)],
            [f["path"] for f in rg["files"]]]
    rg2, ro2 = run_both(tmp_path, "rt2", runs, bottommost_level=1,
                        compression=1)
    survivors = []
    for f in ro2["files"]:
        with open(f["path"], "rb") as fh:
            survivors += oracle.read_sst(fh.read())
    vals = {k[:-8]: v for k, v in survivors}
    assert vals[far_key] == bb.shapes()["far201k"]
    assert bb.k16(10 * (37 + 61) + 5) not in vals


def test_pool_reuse_large_small_large(tmp_path):
    """The buffer-capacity class of test_bbt_dzt_bbt_outoff_realloc: the
    compressed-output slots shrink and grow between jobs on one pooled
    worker."""
    large = kib_values_runs(tmp_path, 300, 150, 0x9001)
    rng = random.Random(0x9002)
    small = [[bb.write_run(tmp_path, "small.sst",
                           [(bb.k16(i), 1 + i, V, small_value(rng))
                            for i in range(2000)])]]
    for tag, runs, bs in (("p1", large, 65536), ("p2", small, 4096),
                          ("p3", large, 65536)):
        run_both(tmp_path, tag, runs, bottommost_level=1, compression=1,
                 block_size=bs)


_child_died = []


@pytest.mark.parametrize("val", ["1", "2", "3"])
def test_compress_variant_skips_large_blocks(tmp_path, val):
    """DCW_COMPRESS_V picks the kernel for blocks up to 16 KiB; every
    variant leaves the larger ones to k_compress_large.  The variable is
    read once per process, so the job runs in a child."""
    if _child_died:
        pytest.fail("an earlier variant child died: " + _child_died[0])
    runs = shapes_runs(tmp_path)
    kw = dict(bottommost_level=1, compression=1)
    oo = tmp_path / "o"
    oo.mkdir()
    ro = oracle.execute(oracle.make_job(runs, str(oo), **kw))
    manifest = {"result": str(tmp_path / "result.json"),
                "jobs": [dict(name="shapes", runs=runs, kw=kw,
                              out_dir=str(tmp_path / "g"))]}
    mpath = tmp_path / "manifest.json"
    mpath.write_text(json.dumps(manifest))
    env = dict(os.environ, DCW_COMPRESS_V=val)
    try:
        r = subprocess.run([sys.executable, RUNNER, str(mpath)], env=env,
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _child_died.append("DCW_COMPRESS_V=%s timed out" % val)
        pytest.fail(_child_died[0])
    if r.returncode != 0:
        _child_died.append("DCW_COMPRESS_V=%s exited %d" % (val, r.returncode))
        pytest.fail(_child_died[0] + "\n" + r.stdout[-2000:] + r.stderr[-4000:])
    with open(manifest["result"]) as f:
        rg = json.load(f)["shapes"]
    assert "error" not in rg, rg
    assert rg["out_entries"] == ro["out_entries"]
    assert len(rg["files"]) == len(ro["files"])
    for fg, fo in zip(rg["files"], ro["files"]):
        with open(fg["path"], "rb") as a, open(fo["path"], "rb") as b:
            assert a.read() == b.read(), fg["path"]


def test_general_keys_one_large_value(tmp_path):
    rng = random.Random(0x6E4)
    kvs, seq = [], 1
    for _ in range(400):
        ln = rng.choice([6, 10, 16, 24, 33, 48])
        kvs.append((rng.randbytes(ln), seq, V, small_value(rng)))
        seq += 1
    kvs = list({k: (k, s, t, v) for k, s, t, v in kvs}.values())
    kvs.append((b"\x80" + rng.randbytes(30), seq, V,
                bb.shapes()["periodic70k"]))
    runs = [[bb.write_run(tmp_path, "g0.sst", kvs[0::2])],
            [bb.write_run(tmp_path, "g1.sst", kvs[1::2])]]
    _, ro = run_both(tmp_path, "gen", runs, bottommost_level=1, compression=1)
    assert any(btype == 1 and unc > 70810
               for _, _, btype, unc in oracle_blocks(ro))
