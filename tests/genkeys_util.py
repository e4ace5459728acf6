"""Helpers shared by the general-key DcwZipTable and range-deletion GPU tests:
input writers, the GPU-against-oracle whole-file compare, and a plain
Python count of what a range-deletion job must keep."""
import oracle
import toplingdb_amd as dcw


def ikey_sort(kvs):
    """(user key, seq, type, value) in internal-key order."""
    return sorted(kvs, key=lambda e: (e[0], -((e[1] << 8) | e[2])))


def write_sst(tmp_path, name, kvs, tombstones=()):
    es = [(oracle.make_ikey(k, s, t), v) for k, s, t, v in ikey_sort(kvs)]
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(oracle.build_sst(es, tombstones=tombstones))
    return p


def fresh(tmp_path, name):
    d = tmp_path / name
    d.mkdir()
    return str(d)


def _twins(tmp_path, runs, tag):
    """The oracle reads no DZT inputs: it gets each DZT file's
    BlockBasedTable twin, the same entry stream (dzt_foreign.twin_sst)."""
    import dzt_foreign
    out = []
    for r, files in enumerate(runs):
        tr = []
        for i, p in enumerate(files):
            if is_dzt(p):
                t = str(tmp_path / ("twin%s_%d_%d.sst" % (tag, r, i)))
                with open(t, "wb") as f:
                    f.write(dzt_foreign.twin_sst(p))
                p = t
            tr.append(p)
        out.append(tr)
    return out


def run_both(tmp_path, runs, tag="", **kw):
    """The job on the GPU worker and on the oracle: whole files byte for
    byte, plus file count, boundary keys and entry counts."""
    rg = dcw.execute(dcw.make_job(runs, fresh(tmp_path, "g" + tag), **kw))
    ro = oracle.execute(oracle.make_job(_twins(tmp_path, runs, tag),
                                        fresh(tmp_path, "o" + tag), **kw))
    assert rg["out_entries"] == ro["out_entries"]
    assert len(rg["files"]) == len(ro["files"])
    for fg, fo in zip(rg["files"], ro["files"]):
        with open(fg["path"], "rb") as a, open(fo["path"], "rb") as b:
            da, db = a.read(), b.read()
        assert da == db, "%s differs from the oracle's (%d vs %d bytes)" % (
            fg["path"], len(da), len(db))
        assert fg["smallest"] == fo["smallest"]
        assert fg["largest"] == fo["largest"]
        assert fg["num_entries"] == fo["num_entries"]
        assert fg["smallest_seqno"] == fo["smallest_seqno"]
        assert fg["largest_seqno"] == fo["largest_seqno"]
    return rg, ro


def is_dzt(path):
    with open(path, "rb") as f:
        return f.read()[-8:] == b"DCWZIP01"


def dzt_ukey_len(path):
    import dzt_foreign
    with open(path, "rb") as f:
        return dzt_foreign.Dzt(f.read()).U


def rangedel_survivors(kvs, tombstones):
    """Entries a bottommost job without snapshots keeps when every entry is
    a Put: one per user key, unless a tombstone [start, end) holding the key
    has a seq above the key's newest version (bytes compare in raw bytewise
    order, as the comparator does)."""
    newest = {}
    for k, s, t, _ in kvs:
        assert t == 1
        newest[k] = max(newest.get(k, 0), s)
    return sum(1 for k, s in newest.items()
               if not any(a <= k < b and ts > s for a, b, ts in tombstones))
