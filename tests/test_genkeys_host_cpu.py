"""General-key range-tombstone lookup and DcwZipTable key records, without a
GPU.

tools/gk_host compiles the source the kernels run: bound_cmp / rd_frag_upper
(dcw_bound_cmp.h, behind fsm_rd_covers) and the key-record writer
(dcw_dzt_enc.h, behind k_dzt_keys_g), with fragment_tombstones and
dzt_plan_files from dcw_host.cpp.  It is built with
-fsanitize=address,undefined as a stand-alone program.

Fragment coverage: for every probe key the program prints the max seq of the
fragment that contains it; the expected value is a brute-force scan over the
tombstones here (Python bytes compare in raw bytewise order).  Corpus: the
prefix-tie keys that the zero-padded words cannot order, bounds that differ
only past byte 16 (fast and general mode) and only past byte 48.

Key area: the oracle writes DZT files; their survivors, read back through
dzt_foreign.Dzt, are the program's input; the key area and key index it
writes in the kernel's per-block schedule must equal the oracle file's.
"""
import os
import shutil
import struct
import subprocess
import sys

import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dzt_foreign as dzf  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TIES = [b"ab", b"ab\x00", b"ab\x00x", b"abc", b"ab" + b"\x00" * 20,
        b"ab" + b"\x00" * 20 + b"x"]


@pytest.fixture(scope="module")
def gk_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not installed")
    exe = tmp_path_factory.mktemp("gk_host") / "gk_host"
    csrc = os.path.join(REPO, "toplingdb_amd", "csrc")
    r = subprocess.run(
        ["g++", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-I", csrc, "-o", str(exe),
         os.path.join(REPO, "tools", "gk_host", "gk_host.cpp"),
         os.path.join(csrc, "dcw_host.cpp"), "-l:libzstd.so.1"],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


def _lp(b):
    return struct.pack("<I", len(b)) + b


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert lines[-2:] == ["OK", ""]
    return lines[:-2]


def brute(tombstones, probe):
    return max([seq for s, e, seq in tombstones if s <= probe < e],
               default=0)


def check_frags(exe, tmp_path, name, general, tombstones, probes):
    job = bytearray(b"GKFR") + struct.pack("<II", general, len(tombstones))
    for s, e, seq in tombstones:
        job += _lp(s) + _lp(e) + struct.pack("<Q", seq)
    job += struct.pack("<I", len(probes))
    for p in probes:
        job += _lp(p)
    path = tmp_path / (name + ".gkfr")
    path.write_bytes(bytes(job))
    got = [int(x) for x in _run(exe, path)]
    want = [brute(tombstones, p) for p in probes]
    assert got == want, (name, [p for p, g, w in zip(probes, got, want)
                                if g != w])
    return got


def around(keys, maxlen):
    """Probe keys at and next to every bound: the bound cut to the job-key
    envelope, its successor key, its predecessor."""
    out = set()
    for k in keys:
        c = k[:maxlen]
        out.add(c)
        if len(c) < maxlen:
            out.add(c + b"\x00")
        if c and c[-1] > 0:
            out.add(c[:-1] + bytes([c[-1] - 1]))
        if c and c[-1] < 255:
            out.add(c[:-1] + bytes([c[-1] + 1]))
        out.add(c[:-1])
    out.discard(b"")
    return sorted(out)


def test_fragment_coverage_prefix_ties(gk_host, tmp_path):
    pairs = [(s, e) for s in TIES for e in TIES if s < e]
    assert len(pairs) == 15
    probes = around(TIES, 48)
    fast_probes = [p for p in probes if len(p) <= 16]
    assert set(TIES) <= set(probes) and len(fast_probes) >= 6
    hit = 0
    for i, (s, e) in enumerate(pairs):
        ts = [(s, e, 100 + i)]
        hit += sum(g > 0 for g in check_frags(gk_host, tmp_path, "g%d" % i, 1,
                                              ts, probes))
        # fast mode: job keys of <= 16 bytes against the same (longer) bounds
        check_frags(gk_host, tmp_path, "f%d" % i, 0, ts, fast_probes)
    assert hit >= 15
    allts = [(s, e, 100 + 7 * i % 15) for i, (s, e) in enumerate(pairs)]
    check_frags(gk_host, tmp_path, "gall", 1, allts, probes)
    check_frags(gk_host, tmp_path, "fall", 0, allts, fast_probes)


def test_fragment_coverage_bounds_past_the_stored_bytes(gk_host, tmp_path):
    p16 = b"k%015d" % 7
    p48 = b"q%047d" % 7
    # two starts that tie on the words, two that tie on the first 48 bytes
    a17, b17 = p16 + b"a", p16 + b"b"
    a49, b49 = p48 + b"a", p48 + b"b"
    ts = [(a17, b17, 50), (b17, p16 + b"c", 60), (b"k", a17, 40),
          (a49, b49, 70), (b49, p48 + b"c" * 12, 80), (b"q", a49, 30)]
    probes = around([a17, b17, p16, a49, b49, p48, b"k", b"q"], 48)
    got = check_frags(gk_host, tmp_path, "gen", 1, ts, probes)
    assert {30, 40, 50, 60, 0} <= set(got)
    fast = around([a17, b17, p16, b"k", b"q", a49], 16)
    got = check_frags(gk_host, tmp_path, "fast", 0, ts, fast)
    # no key of <= 16 bytes lies inside [a17, p16 + "c"): seqs 50, 60 unseen
    assert {30, 40, 0} <= set(got)
    # each pair alone too: a search that confused the tied starts would still
    # pass with a neighbour of the same seq next to it
    for i, t in enumerate(ts):
        check_frags(gk_host, tmp_path, "gen%d" % i, 1, [t], probes)
        check_frags(gk_host, tmp_path, "fast%d" % i, 0, [t], fast)


def _survivors(path):
    z = dzf.Dzt(open(path, "rb").read())
    recs = []
    for kb in range(len(z.kblocks)):
        for key, tag, _voff, vlen in dzf._records(z, kb):
            recs.append((key + struct.pack("<Q", tag), vlen))
    kindex = b"".join(bytes(fk) + struct.pack("<QIQ", koff, ksize, fr)
                      for fk, koff, ksize, fr in z.kblocks)
    return z, recs, kindex


@pytest.mark.parametrize("U", [8, 17, 24, 48])
def test_key_area_matches_oracle(gk_host, tmp_path, U):
    # 700 user keys with a 3-byte varying tail after a long common prefix;
    # every third key has two versions on either side of a snapshot, so both
    # survive and the second shares all U key bytes (the clamp)
    entries = []
    for i in range(700):
        uk = (b"%0" + str(U).encode() + b"d") % (i * 7)
        seqs = [2000 + i, 100 + i] if i % 3 == 0 else [100 + i]
        for s in seqs:
            entries.append((oracle.make_ikey(uk, s, 1),
                            b"v" * (1 + (i * 37 + s) % 90)))
    target = 16 << 10
    paths = dzf.oracle_dzt(tmp_path, "u%d" % U, entries, bottommost_level=0,
                           snapshots=[1000], target_file_size=target)
    assert len(paths) >= 3
    files = [_survivors(p) for p in paths]
    recs = [r for _, rs, _ in files for r in rs]
    assert len(recs) == len(entries)
    assert [k for k, _ in recs] == [k for k, _ in entries]
    job = bytearray(b"GKKA") + struct.pack("<IQI", U, target, len(recs))
    for ik, vlen in recs:
        assert len(ik) == U + 8
        job += ik + struct.pack("<I", vlen)
    jpath = tmp_path / "job.gkka"
    jpath.write_bytes(bytes(job))
    opath = tmp_path / "out.bin"
    assert _run(gk_host, jpath, opath) == ["files %d" % len(paths)]
    out = opath.read_bytes()
    (nf,) = struct.unpack_from("<I", out, 0)
    assert nf == len(paths)
    at = 4
    for z, _, kindex in files:
        (n,) = struct.unpack_from("<Q", out, at)
        at += 8
        assert out[at:at + n] == bytes(z.key_area)
        at += n
        (n,) = struct.unpack_from("<Q", out, at)
        at += 8
        assert out[at:at + n] == kindex
        at += n
        assert len(z.kblocks) >= 2
    assert at == len(out)
