"""The boundary corpus (tests/bounds_corpus.py) on the CPU: the oracle agrees
with the plain-Python model, and every job can tell raw bytewise order of
its boundaries from a compare of zero-padded 16-byte words.

The second point is a condition on the corpus, not a measurement: a job of
a SEPARATING group whose result does not change under the padded compare
could not fail on a worker that compares that way, and is worth nothing in
tests/test_bounds_gpu.py."""
import os
import sys

import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds_corpus as bc  # noqa: E402


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("bounds")


def run_oracle(workdir, job, kw, tag):
    out = os.path.join(str(workdir), "%s_%s" % (job.name, tag))
    os.makedirs(out)
    return oracle.execute(oracle.make_job(job.write_inputs(workdir), out, **kw))


def read_back(res):
    got = []
    for f in res["files"]:
        with open(f["path"], "rb") as fh:
            got += oracle.read_sst(fh.read())
    return got


def cut_keys(res):
    return [(f["smallest"], f["largest"]) for f in res["files"]]


_results = {}


def both_runs(workdir, job):
    """(raw-order result, padded-compare result) of the oracle, once."""
    if job.name not in _results:
        _results[job.name] = (run_oracle(workdir, job, job.kw(), "raw"),
                              run_oracle(workdir, job, job.legacy_kw(), "pad"))
    return _results[job.name]


def test_legacy_bound_is_the_padded_compare():
    # legacy_bound(b, U) must order against every U-byte key as the
    # zero-padded 16-byte words of b and of the key do
    for u in (8, 16):
        keys = [bytes([97 + i]) * (u - 2) + t
                for i in range(3) for t in (b"\0\0", b"\0a", b"a\0", b"aa")]
        bounds = [k[:n] for k in keys for n in range(u - 3, u + 1)]
        bounds += [k + t for k in keys
                   for t in (b"\0", b"\0\0", b"x", b"\0x", b"x" * 9)]
        for b in bounds:
            lb = bc.legacy_bound(b, u)
            for k in keys:
                padded = (bc.pad16(b) > bc.pad16(k)) - (bc.pad16(b) < bc.pad16(k))
                assert ((lb > k) - (lb < k)) == padded, (b, k)
        assert bc.legacy_bound(b"k" * 16 + b"x", 16) == b"k" * 16
        assert bc.legacy_bound(b"k" * 14, 16) == b"k" * 14 + b"\0\0"


def test_corpus_has_every_group():
    groups = {j.group for j in bc.all_jobs()}
    assert groups == set(bc.SEPARATING) | set(bc.NON_SEPARATING) | {"switch"}
    assert len(set(bc.names(bc.all_jobs()))) == len(bc.all_jobs())


@pytest.mark.parametrize("name", bc.names(bc.all_jobs()))
def test_oracle_matches_model(workdir, name):
    job = bc.by_name(name)
    res, _ = both_runs(workdir, job)
    got = read_back(res)
    assert res["out_entries"] == len(got)
    if job.model:
        assert got == job.expected
    else:  # oracle only: at least sorted, and something dropped
        assert 0 < len(got) < sum(len(r) for r in job.kvs_runs)


@pytest.mark.parametrize("name", bc.names(bc.all_jobs()))
def test_discrimination(workdir, name):
    job = bc.by_name(name)
    if job.group == "switch":
        return  # boundaries are not looked at
    raw, pad = both_runs(workdir, job)
    if job.grandparents:
        assert len(raw["files"]) > 1, "no cut at all"
        assert read_back(raw) == read_back(pad) == job.expected
        differs = cut_keys(raw) != cut_keys(pad)
    elif job.model and job.ulen == 0:
        # general mode cuts the job key to 16 bytes too: Python model of it
        assert read_back(pad) == job._survivors(lambda k: any(
            bc.legacy_bound(sm, 0) <= k <= bc.legacy_bound(lg, 0)
            for lv in job.levels for sm, lg in lv))
        differs = job.legacy_expected != job.expected
    else:
        if job.model:
            assert read_back(pad) == job.legacy_expected
        differs = read_back(raw) != read_back(pad)
    assert differs == (job.group in bc.SEPARATING), (
        "group %r: padded compare gives %s result" %
        (job.group, "another" if differs else "the same"))


@pytest.mark.parametrize("name", [j.name for j in bc.level_below_jobs()
                                  if j.model])
def test_tombstones_kept_and_dropped(name):
    job = bc.by_name(name)
    kept = [k for k, v in job.expected if k[-8] != bc.TYPE_VALUE]
    assert len(job.tombstones) >= 10
    if job.name == "switch_levels_below_invalid":
        assert len(kept) == len(job.tombstones)
    elif job.name == "switch_bottommost":
        assert kept == []
    else:
        assert 0 < len(kept) < len(job.tombstones)
    assert any(k[-8] == bc.TYPE_VALUE for k, v in job.expected)
