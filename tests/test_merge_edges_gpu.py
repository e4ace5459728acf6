"""Merge and dedup at the kernels' own edges: small bottommost jobs whose
entry, group and run counts sit on the constants of the merge and scan
kernels (dcw_k_merge.h): MT_TILE = 2048 output entries per workgroup of
k_merge_tiled, 8 per thread; scan blocks of 1024 (k_scan_partial /
k_scan_add_base, k_build_headidx); the odd-run copy-through of
GpuJob::merge.

Each job is checked twice, both exactly: output files bit-identical to the
oracle's, and read back equal to the survivor list computed in plain Python
(newest version of each user key; a Delete vanishes with what it covers).
The whole set runs again in two fresh child processes, one with the
tile-boundary precompute switched off (DCW_MERGE_V=0, read once per
process) and one with the variable stripped.
"""
import functools
import json
import os
import random
import subprocess
import sys

import pytest

import oracle
import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import foreign_corpus as fc  # noqa: E402

pytestmark = pytest.mark.gpu

JOB_KW = dict(compression=0, bottommost_level=1)
RUNNER = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      "foreign_variant_runner.py")
DEL, PUT = fc.TYPE_DELETION, fc.TYPE_VALUE
TILE, PER_THREAD, SCAN = 2048, 8, 1024


def put(i, seq, key=fc.ukey):
    return (key(i), seq, PUT, b"v%d-%d" % (i, seq))


def split_job(total, n_a, rng, order="mixed"):
    """`total` distinct keys, all Puts; `n_a` of them in run A."""
    if order == "mixed":
        in_a = set(rng.sample(range(total), n_a))
    elif order == "a_below_b":
        in_a = set(range(n_a))
    else:  # a_above_b
        in_a = set(range(total - n_a, total))
    a = [put(i, 1 + i) for i in range(total) if i in in_a]
    b = [put(i, 1 + i) for i in range(total) if i not in in_a]
    return [a, b]


def straddle_job(newer_in, newer_type, rng):
    """One version per user key, but two keys with one version in each run,
    placed so that the pair takes output positions 999|1000 (a thread's
    8-entry boundary inside a tile) and 2047|2048 (the tile edge).  The
    newer version sorts first whichever run holds it."""
    nkeys = 3000
    # key j < 999 is at position j; key 999 takes 999 and 1000; key j > 999
    # starts at j + 1, so key 2046 takes 2047 and 2048
    doubles = (999, TILE - 2)
    assert (doubles[0] + 1) % PER_THREAD == 0 and doubles[1] + 2 == TILE
    runs = [[], []]
    for j in range(nkeys):
        if j in doubles:
            v = b"" if newer_type == DEL else b"newer-%d" % j
            runs[newer_in].append((fc.ukey(j), 50000 + j, newer_type, v))
            runs[1 - newer_in].append(put(j, 1 + j))
        else:
            runs[rng.randrange(2)].append(put(j, 1 + j))
    return runs


def multi_run_job(sizes, rng, key=fc.ukey):
    """Runs of unequal sizes over one key space; later runs are newer and
    delete a quarter of what they write."""
    space = sum(sizes) * 2 // 3  # a third of the entries shadow another
    runs = []
    for r, n in enumerate(sizes):
        kvs = []
        for i in sorted(rng.sample(range(space), n)):
            seq = 1 + r * 100000 + i
            if r and rng.random() < 0.25:
                kvs.append((key(i), seq, DEL, b""))
            else:
                kvs.append(put(i, seq, key))
        runs.append(kvs)
    return runs


def gkey(i):
    """Mixed lengths with a common 16-byte prefix: general-key mode."""
    return b"g" * 16 + (b"%06d" % i) * (1 + i % 5)


def count_job(groups, extra, rng):
    """`groups` user keys, `extra` of them with a second, older version."""
    runs = [[], []]
    twice = set(rng.sample(range(groups), extra))
    for j in range(groups):
        r = rng.randrange(2)
        runs[r].append(put(j, 10000 + j))
        if j in twice:
            runs[1 - r].append(put(j, 1 + j))
    return runs


@functools.lru_cache(maxsize=None)
def edge_jobs():
    """-> {name: runs}, runs = [[(ukey, seq, type, value)]] sorted."""
    rng = random.Random(0xED6E)
    jobs = {}
    for total in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE,
                  2 * TILE + 1):
        for n_a in (1, 7, 8, 9, total // 2):
            jobs["split_%d_%d" % (total, n_a)] = split_job(total, n_a, rng)
    # a tile's whole segment on one side
    jobs["a_below_b"] = split_job(2 * TILE + 1, TILE + 5, rng, "a_below_b")
    jobs["a_above_b"] = split_job(2 * TILE + 1, TILE + 5, rng, "a_above_b")
    for newer_in in (0, 1):
        for tname, typ in (("put", PUT), ("delete", DEL)):
            jobs["straddle_newer_in_%s_%s" % ("ab"[newer_in], tname)] = \
                straddle_job(newer_in, typ, rng)
    # odd run counts: the leftover run is copied through at each level
    jobs["runs_3"] = multi_run_job((1500, 700, 2300), rng)
    jobs["runs_5"] = multi_run_job((900, 2100, 1, 1300, 500), rng)
    jobs["runs_7"] = multi_run_job((300, 1100, 2049, 7, 800, 1, 1500), rng)
    jobs["runs_5_general"] = multi_run_job((900, 2100, 1, 1300, 500), rng,
                                           gkey)
    for n in (SCAN - 1, SCAN, SCAN + 1):
        jobs["entries_%d" % n] = count_job(n, 0, rng)      # groups == entries
        jobs["groups_%d" % n] = count_job(n, 100, rng)     # entries = n + 100
        jobs["entries_%d_groups_less" % n] = count_job(n - 100, 100, rng)
    for runs in jobs.values():
        for kvs in runs:
            kvs.sort(key=lambda e: (e[0], -((e[1] << 8) | e[2])))
    return jobs


@pytest.fixture(scope="module", autouse=True)
def gpu():
    dcw.init(0)
    yield
    dcw.shutdown()


@pytest.fixture(scope="module")
def prepared(tmp_path_factory):
    """Inputs, oracle outputs and expectations of every job, made once."""
    d = tmp_path_factory.mktemp("merge_edges")
    out = {}
    for name, kvs_runs in edge_jobs().items():
        runs = []
        for r, kvs in enumerate(kvs_runs):
            p = str(d / ("%s_in%d.sst" % (name, r)))
            with open(p, "wb") as f:
                f.write(oracle.build_sst(
                    [(oracle.make_ikey(k, s, t), v) for k, s, t, v in kvs]))
            runs.append([p])
        o = d / (name + "_orc")
        o.mkdir()
        ro = oracle.execute(oracle.make_job(runs, str(o), **JOB_KW))
        out[name] = (runs, ro, fc.survivors(kvs_runs))
    return out


def check(rg, ro, expected, name):
    assert rg["out_entries"] == ro["out_entries"] == len(expected), name
    assert len(rg["files"]) == len(ro["files"]), name
    got = []
    for fg, fo in zip(rg["files"], ro["files"]):
        assert fg["file_number"] == fo["file_number"]
        with open(fg["path"], "rb") as a, open(fo["path"], "rb") as b:
            da, db = a.read(), b.read()
        assert da == db, (name, fg["path"])
        got += oracle.read_sst(da)
    assert got == expected, name


def test_the_jobs_sit_on_the_edges():
    jobs = edge_jobs()
    totals = {sum(len(r) for r in runs) for n, runs in jobs.items()
              if n.startswith("split_")}
    assert totals == {2047, 2048, 2049, 4095, 4096, 4097}
    for name in ("straddle_newer_in_a_put", "straddle_newer_in_b_delete"):
        merged = sorted((e for r in jobs[name] for e in r),
                        key=lambda e: (e[0], -((e[1] << 8) | e[2])))
        for at in (1000, TILE):  # the pair sits on both sides of the edge
            assert at % PER_THREAD == 0
            assert merged[at - 1][0] == merged[at][0]
            assert merged[at - 1][1] > merged[at][1]
    for n in (SCAN - 1, SCAN, SCAN + 1):
        assert sum(len(r) for r in jobs["entries_%d" % n]) == n
        assert len({e[0] for r in jobs["groups_%d" % n] for e in r}) == n
        assert sum(len(r) for r in jobs["entries_%d_groups_less" % n]) == n


@pytest.mark.parametrize("name", sorted(edge_jobs()))
def test_merge_edge(tmp_path, prepared, name):
    runs, ro, expected = prepared[name]
    rg = dcw.execute(dcw.make_job(runs, str(tmp_path), **JOB_KW))
    check(rg, ro, expected, name)


# ---- the whole set in fresh child processes
CHILD_TIMEOUT_S = 120
_child_died = []  # once a child dies no further child is started


@pytest.mark.parametrize("merge_v", [None, "0"],
                         ids=["DCW_MERGE_V-unset", "DCW_MERGE_V=0"])
def test_merge_variant(tmp_path, prepared, merge_v):
    if _child_died:
        pytest.skip("an earlier merge-variant child died: " + _child_died[0])
    manifest = {"result": str(tmp_path / "result.json"), "jobs": []}
    for name, (runs, ro, expected) in prepared.items():
        manifest["jobs"].append(dict(name=name, runs=runs, kw=JOB_KW,
                                     out_dir=str(tmp_path / (name + "_gpu"))))
    mpath = tmp_path / "manifest.json"
    mpath.write_text(json.dumps(manifest))
    env = {k: v for k, v in os.environ.items() if k != "DCW_MERGE_V"}
    if merge_v is not None:
        env["DCW_MERGE_V"] = merge_v
    label = "DCW_MERGE_V=%s" % merge_v
    try:
        r = subprocess.run([sys.executable, RUNNER, str(mpath)], env=env,
                           capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _child_died.append(label + " timed out")
        pytest.fail(_child_died[0])
    if r.returncode != 0:
        _child_died.append("%s exited %d" % (label, r.returncode))
        pytest.fail(_child_died[0] + "\n" + r.stdout[-2000:] + r.stderr[-4000:])
    with open(manifest["result"]) as f:
        results = json.load(f)
    errors = {n: x["error"] for n, x in results.items() if "error" in x}
    if errors:
        _child_died.append("%s job failed: %r" % (label, errors))
        pytest.fail(_child_died[0])
    assert set(results) == set(prepared)
    for name, (runs, ro, expected) in prepared.items():
        check(results[name], ro, expected, name)
