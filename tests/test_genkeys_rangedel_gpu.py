"""Range deletions for any key shape and any bound length (bottommost, no
snapshots, no grandparents): general-key jobs with tombstones, and fast-mode
jobs whose tombstone bounds are longer than 16 bytes.  Every job is compared
with the oracle's on whole files byte for byte; every job also asserts the
number of entries kept against a plain Python count (covered keys with a
seq above the tombstone's survive, those below drop)."""
import os
import random
import sys

import pytest

import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from genkeys_util import (dzt_ukey_len, is_dzt, rangedel_survivors,  # noqa: E402
                          run_both, write_sst)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    dcw.init(0)
    yield
    dcw.shutdown()


def check(tmp_path, runs_kvs, tag="", **kw):
    """runs_kvs: [(kvs, tombstones)] per run."""
    runs = [[write_sst(tmp_path, "in%s_%d.sst" % (tag, r), kvs, ts)]
            for r, (kvs, ts) in enumerate(runs_kvs)]
    rg, _ = run_both(tmp_path, runs, tag=tag, bottommost_level=1, **kw)
    allkv = [e for kvs, _ in runs_kvs for e in kvs]
    allts = [t for _, ts in runs_kvs for t in ts]
    want = rangedel_survivors(allkv, allts)
    assert rg["out_entries"] == want
    return rg, len({k for k, _, _, _ in allkv}) - want


# 1. uniform long keys, three runs, tombstones across runs
@pytest.mark.parametrize("U", [24, 48])
def test_uniform_long_keys_fuzz(tmp_path, U):
    K = lambda i: (b"k%0" + str(U - 1).encode() + b"d") % i
    rnd = random.Random(17 + U)
    runs, seq = [], 1
    for r in range(3):
        kvs = {}
        for _ in range(8000):
            k = K(rnd.randrange(30000))
            kvs[k] = (k, seq, 1, b"v%d" % seq)
            seq += 1
        ts = []
        for _ in range(1 + rnd.randrange(3)):
            a = rnd.randrange(30000)
            ts.append((K(a), K(a + rnd.randrange(1, 4000)), seq))
            seq += 1
        runs.append((list(kvs.values()), ts))
    _, dropped = check(tmp_path, runs, compression=1)
    assert dropped > 100


# 2. mixed-length keys, bounds of several shapes
def test_mixed_length_keys(tmp_path):
    rnd = random.Random(23)
    keys = sorted({bytes(rnd.choice(b"abcdefgh") for _ in range(ln))
                   for ln in (6, 16, 17, 24, 33, 48) for _ in range(700)})
    assert {len(k) for k in keys} == {6, 16, 17, 24, 33, 48}
    runs, seq = [], 1
    for r in range(2):
        kvs = []
        for k in rnd.sample(keys, 2500):
            kvs.append((k, seq, 1, b"v%d" % seq))
            seq += 1
        runs.append([kvs, []])
    n = len(keys)
    pick = lambda f: keys[int(f * n)]
    runs[0][1] = [
        (pick(0.05), pick(0.12), seq + 1),               # existing keys
        (pick(0.30)[:3], pick(0.38), seq + 2),           # a 3-byte prefix
        (pick(0.50) + b"\x00", pick(0.58) + b"\x00", seq + 3),  # key + \0
        (pick(0.70), (pick(0.78) + b"z" * 60)[:60], seq + 4),   # 60 bytes
        (pick(0.85), pick(0.90), 1500),                  # older than run 1
    ]
    assert len(runs[0][1][3][1]) == 60
    _, dropped = check(tmp_path, runs)
    assert dropped > 300


# 3. keys that the padded words alone cannot order
TIES = [b"ab", b"ab\x00", b"ab\x00x", b"abc", b"ab" + b"\x00" * 20,
        b"ab" + b"\x00" * 20 + b"x"]


def test_prefix_ties(tmp_path):
    assert sorted(TIES) == [TIES[0], TIES[1], TIES[4], TIES[5], TIES[2],
                            TIES[3]]
    kvs = []
    for i, k in enumerate(TIES):
        kvs.append((k, 10 + i, 1, b"old-%d" % i))
    pairs = [(s, e) for s in TIES for e in TIES if s < e]
    assert len(pairs) == 15
    dropped = []
    for i, (s, e) in enumerate(pairs):
        _, d = check(tmp_path, [(kvs, [(s, e, 500)])], tag="p%d" % i)
        dropped.append(d)
    # [s, e) holds s and every listed key between: 1..5 keys
    assert sorted(set(dropped)) == [1, 2, 3, 4, 5]


# 4. bounds that differ only past the bytes the device keeps
def test_bounds_differing_past_byte_16_and_48(tmp_path):
    p16 = b"k%015d" % 7
    p48 = b"q%047d" % 7
    a17, b17, c17 = p16 + b"a", p16 + b"b", p16 + b"c"
    a49, b49 = p48 + b"a", p48 + b"b"
    keys = [p16, a17, a17 + b"\x00", a17 + b"zzz", b17, b17 + b"x" * 20, c17,
            p16 + b"d" * 8, p16[:15], p16[:15] + b"8",
            p48, p48[:47], p48[:47] + b"8", p48[:40], b"q", b"r" * 30]
    kvs = [(k, 100 + i, 1, b"v%d" % i) for i, k in enumerate(keys)]
    cases = [
        [(a17, b17, 900)],                      # holds a17, a17\0, a17zzz
        [(b17, c17, 900)],                      # holds b17, b17xxx...
        [(a17, b17, 900), (b17, c17, 50)],      # second one too old to drop
        [(a49, b49, 900)],                      # no job key can be inside
        [(p48[:47], a49, 900)],                 # holds p48[:47] and p48
        [(b49, b"r", 900)],                     # starts past p48
        [(b"k", a17, 900), (a49, b49 + b"x" * 11, 900)],  # p16[:15], p16
    ]
    want_dropped = [3, 2, 3, 0, 2, 1, 2]
    got = []
    for i, ts in enumerate(cases):
        _, d = check(tmp_path, [(kvs, ts)], tag="c%d" % i)
        got.append(d)
    assert got == want_dropped


# 5. fast mode (16-byte keys) with bounds longer than 16 bytes
def test_fast_mode_long_bounds(tmp_path):
    K = lambda i: b"k%015d" % i
    kvs = [(K(i), 100 + i, 1, b"v%d" % i) for i in range(5000)]
    ts = [(K(100) + b"x", K(200) + b"y" * 24, 900_000),   # 17 and 40 bytes
          (K(1000) + b"\x00", K(1000) + b"\x00\x00", 900_001),  # holds none
          (K(3000), K(3100) + b"a", 900_002),             # 16 and 17 bytes
          (K(4000) + b"\x00" * 24, K(4001), 50)]          # too old
    assert len(ts[0][0]) == 17 and len(ts[0][1]) == 40
    rg, dropped = check(tmp_path, [(kvs[0::2], ts), (kvs[1::2], [])])
    assert dropped == 100 + 0 + 101 + 0


# 6. general keys, tombstones and DcwZipTable output together
def test_combined_with_dzt_output(tmp_path):
    K = lambda i: b"key-%020d" % i
    kvs = [(K(i), 100 + i, 1, b"val-%d" % i) for i in range(9000)]
    ts = [(K(2000), K(6000) + b"\x00" * 30, 777_000)]
    rg, dropped = check(tmp_path, [(kvs[0::2], ts), (kvs[1::2], [])],
                        compression=1, output_table_factory=1)
    assert dropped == 4001
    assert is_dzt(rg["files"][0]["path"])
    assert dzt_ukey_len(rg["files"][0]["path"]) == 24


# 7. covered keys: a seq above the tombstone's survives, one below drops
@pytest.mark.parametrize("U", [16, 33])
def test_covered_seq_above_and_below(tmp_path, U):
    K = lambda i: (b"k%0" + str(U - 1).encode() + b"d") % i
    tseq = 10_000
    old = [(K(i), 100 + i, 1, b"old") for i in range(3000)]
    new = [(K(i), 20_000 + i, 1, b"new") for i in range(0, 3000, 4)]
    ts = [(K(500), K(2500) + b"\xff" * 20, tseq)]
    rg, dropped = check(tmp_path, [(new, []), (old, ts)])
    inside = range(500, 2501)
    assert dropped == sum(1 for i in inside if i % 4)
    assert rg["out_entries"] == 3000 - dropped
