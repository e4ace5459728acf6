"""DcwZipTable output in general-key mode: jobs whose inputs are not all of
one user-key length <= 16 bytes, but whose SURVIVORS have one length U in
1..48, write DZT files through the side-table key-area kernel.  Every job is
compared with the oracle's on whole files byte for byte, plus file count,
boundary keys and entry counts.  Survivors of more than one length are
refused, as the oracle refuses them."""
import os
import random
import sys

import pytest

import oracle
import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dzt_foreign as zf  # noqa: E402
from genkeys_util import (dzt_ukey_len, fresh, is_dzt, run_both,  # noqa: E402
                          write_sst)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    dcw.init(0)
    yield
    dcw.shutdown()


def key_of(U, cp, j):
    """User key j of U bytes whose common prefix with the other keys is
    exactly cp bytes: the byte after the prefix varies with j."""
    tl = U - cp
    if tl >= 5:
        tail = bytes([j % 251]) + (b"%0" + str(tl - 1).encode() + b"d") % j
    else:
        tail = j.to_bytes(tl, "little")
    return b"P" * cp + tail


def check_dzt(rg, U):
    assert rg["files"]
    for f in rg["files"]:
        assert is_dzt(f["path"])
        assert dzt_ukey_len(f["path"]) == U
        assert len(f["smallest"]) == len(f["largest"]) == U + 8


def puts(U, n, seq0=100, vf=None, cp=3):
    vf = vf or (lambda i: b"val-%d-" % i * (1 + i % 4))
    return [(key_of(U, cp, i), seq0 + i, 1, vf(i)) for i in range(n)]


# 1. key lengths, prefix shapes, compression, two versions of one key
@pytest.mark.parametrize("U,cp", [(17, 5), (17, 15), (24, 5), (24, 16),
                                  (47, 16), (47, 40), (48, 5), (48, 16),
                                  (48, 40)])
def test_key_lengths(tmp_path, U, cp):
    rnd = random.Random(U * 100 + cp)
    space = min(4000, 256 ** min(U - cp, 4))
    runs, seq = [], 1
    for r in range(2):
        kvs = []
        for j in rnd.sample(range(space), 3000):
            t = 0 if rnd.random() < 0.15 else 1
            kvs.append((key_of(U, cp, j), seq, t,
                        b"" if t == 0 else b"value-%d-" % seq * (1 + seq % 5)))
            seq += 1
        runs.append([write_sst(tmp_path, "r%d.sst" % r, kvs)])
    # not bottommost, and a snapshot between the runs: a key present in both
    # keeps both versions, so the second one shares all U key bytes and more
    for comp in (0, 1):
        rg, _ = run_both(tmp_path, runs, tag=str(comp), compression=comp,
                         bottommost_level=0, snapshots=[3000, 4500],
                         output_table_factory=1)
        check_dzt(rg, U)
        got = oracle.dzt_read(open(rg["files"][0]["path"], "rb").read())
        assert any(a[0][:-8] == b[0][:-8] for a, b in zip(got, got[1:]))


# 2. key-block edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129])
def test_key_block_edges(tmp_path, n):
    p = write_sst(tmp_path, "e.sst", puts(24, n))
    rg, _ = run_both(tmp_path, [[p]], compression=1, output_table_factory=1)
    check_dzt(rg, 24)
    assert rg["out_entries"] == n
    z = zf.Dzt(open(rg["files"][0]["path"], "rb").read())
    assert len(z.kblocks) == (n + 63) // 64


# 3. file cuts
def test_file_cuts(tmp_path):
    kvs = puts(33, 6000, vf=lambda i: b"v%039d" % i)
    runs = [[write_sst(tmp_path, "a.sst", kvs[0::2])],
            [write_sst(tmp_path, "b.sst", kvs[1::2])]]
    rg, ro = run_both(tmp_path, runs, compression=1, output_table_factory=1,
                      target_file_size=64 << 10)
    check_dzt(rg, 33)
    assert len(rg["files"]) >= 3
    assert ([(f["smallest"], f["largest"]) for f in rg["files"]] ==
            [(f["smallest"], f["largest"]) for f in ro["files"]])


# 4. one oversize value: a raw single-value block
def test_oversize_value(tmp_path):
    rnd = random.Random(5)
    big = rnd.randbytes(20 << 10)
    kvs = puts(48, 300, vf=lambda i: big if i == 170 else b"small-%d" % i)
    p = write_sst(tmp_path, "big.sst", kvs)
    rg, _ = run_both(tmp_path, [[p]], compression=1, output_table_factory=1)
    check_dzt(rg, 48)
    z = zf.Dzt(open(rg["files"][0]["path"], "rb").read())
    assert [b[2] for b in z.vblocks].count(20 << 10) == 1


# 5. a DZT level compacted into again, then read back by the worker
def test_dzt_level_compacted_into_again(tmp_path):
    old = [(oracle.make_ikey(zf.ukey(i, width=24), 1000 + i, 1),
            b"old-%06d-" % i * 6) for i in range(2000)]
    old_run = zf.oracle_dzt(tmp_path, "old", old)
    assert zf.Dzt(open(old_run[0], "rb").read()).U == 24
    newer = [(zf.ukey(i, width=24), 50_000 + i, 0 if i % 9 == 0 else 1,
              b"" if i % 9 == 0 else b"new-%d" % i) for i in range(0, 2400, 3)]
    bbt = write_sst(tmp_path, "newer.sst", newer)
    # the oracle reads no DZT files: run_both hands it each DZT input's
    # BlockBasedTable twin, the same entry stream (as test_dzt_input_gpu does)
    rg, _ = run_both(tmp_path, [[bbt], old_run], tag="1", compression=1,
                     output_table_factory=1)
    check_dzt(rg, 24)
    # the worker's own DZT file as the only input of the next job
    own = [f["path"] for f in rg["files"]]
    rg2, _ = run_both(tmp_path, [own], tag="2", compression=1)
    assert rg2["out_entries"] == rg["out_entries"]
    assert not is_dzt(rg2["files"][0]["path"])


# 6. uniform survivors from mixed inputs
@pytest.mark.parametrize("keep,drop", [(24, 8), (8, 24)])
def test_uniform_survivors_from_mixed_inputs(tmp_path, keep, drop):
    older = puts(keep, 500, seq0=100) + [
        (key_of(drop, 3, i), 5000 + i, 1, b"gone-%d" % i) for i in range(300)]
    newer = [(key_of(drop, 3, i), 9000 + i, 0, b"") for i in range(300)]
    runs = [[write_sst(tmp_path, "new.sst", newer)],
            [write_sst(tmp_path, "old.sst", older)]]
    rg, _ = run_both(tmp_path, runs, compression=1, bottommost_level=1,
                     output_table_factory=1)
    check_dzt(rg, keep)
    assert rg["out_entries"] == 500


# 7. survivors of two lengths: refused, nothing written, worker intact
def test_non_uniform_survivors_refused(tmp_path):
    kvs = puts(24, 200) + [(key_of(8, 3, i), 900 + i, 1, b"w") for i in range(9)]
    p = write_sst(tmp_path, "mix.sst", kvs)
    out = fresh(tmp_path, "refused")
    with pytest.raises(RuntimeError, match="uniform"):
        dcw.execute(dcw.make_job([[p]], out, output_table_factory=1))
    assert os.listdir(out) == []
    with pytest.raises(RuntimeError, match="uniform"):
        oracle.execute(oracle.make_job([[p]], fresh(tmp_path, "orefused"),
                                       output_table_factory=1))
    q = write_sst(tmp_path, "next.sst", puts(24, 500))
    rg, _ = run_both(tmp_path, [[q]], compression=1, output_table_factory=1)
    check_dzt(rg, 24)


# 8. the fast path through the same helper
def test_fast_path_u16(tmp_path):
    kvs = puts(16, 3000)
    runs = [[write_sst(tmp_path, "a.sst", kvs[0::2])],
            [write_sst(tmp_path, "b.sst", kvs[1::2])]]
    rg, _ = run_both(tmp_path, runs, compression=1, output_table_factory=1)
    check_dzt(rg, 16)
