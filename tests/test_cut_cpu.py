"""The worker's file cutter against the oracle, without a GPU.

tools/cut_host drives FileCutter (dcw_host.h) the way the worker does: host
block planning, one cutter call per chunk, advance.  It is built with
-fsanitize=address,undefined as a stand-alone program.  For every job the
oracle (oracle/compact.c out_should_stop_before, an independent
implementation) writes its output files; the survivors read back from them
are the program's input, and the program's files must match the oracle's
one for one on count, smallest, largest and entries per file.

Corpus: every grandparent job of tests/bounds_corpus.py (target 1 MiB, about
0.9 MiB of output: the "cut" shapes are cut by max_compaction_bytes, the
"dyn" shapes by the dynamic file size rule), and two jobs without
grandparents whose small target makes the size-only path cut several times.
"""
import os
import shutil
import struct
import subprocess
import sys

import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds_corpus as bc  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = ("size", "max_compaction_bytes", "dynamic")


def _size_job(name, key, ulen, target):
    """GP_ENTRIES Puts in two runs, no grandparents: about 0.9 MiB of output
    against a target of a few hundred KiB."""
    kvs = [(key(i), 1 + i, bc.TYPE_VALUE, bc._gp_value(i))
           for i in range(bc.GP_ENTRIES)]
    return bc.Job(name, "size", [kvs[0::2], kvs[1::2]], ulen=ulen,
                  target_file_size=target)


def _stride_job():
    """Grandparent cuts at block boundaries.  The corpus jobs cross their
    boundaries at arbitrary places of a block.  Here adjacent grandparent
    files of 1 MiB tile the key space, file j+1 starting d entries after file
    j, against a budget of 1.5 MiB: every file start is crossed with 2 MiB
    counted and cuts the output there, and the new output file starts a new
    block at that entry.  Entries take 110 to 120 bytes of a 4 KiB block, so
    a block holds between 28 and 44 of them; d runs through all of 28..44
    twice, so some cut follows the one before it by exactly one block."""
    starts, g = [], 60
    for d in 2 * list(range(28, 45)):
        starts.append(g)
        g += d
    n = g + 60
    kvs = [(bc.k16(i), 1 + i, bc.TYPE_VALUE, bc._gp_value(i))
           for i in range(n)]
    gps = [(bc.k16(a), bc.k16(b - 1), bc.MIB)
           for a, b in zip(starts, starts[1:] + [n + 10])]
    return bc.Job("gp16_stride_cut", "gp_same", [kvs[0::2], kvs[1::2]],
                  grandparents=gps, target_file_size=bc.MIB,
                  max_compaction_bytes=3 * bc.MIB // 2)


def jobs():
    return list(bc.grandparent_jobs()) + [
        _stride_job(),
        _size_job("size16_256k", bc.k16, 16, 256 << 10),
        _size_job("size8_300k", bc.k8, 8, 300000),
    ]


def _lp(b):
    return struct.pack("<I", len(b)) + b


def job_file(desc, grandparents, survivors):
    out = bytearray(b"DCUT")
    out += struct.pack("<QQ6I", desc.target_file_size,
                       desc.max_compaction_bytes,
                       desc.level_compaction_dynamic_file_size,
                       desc.block_size, desc.block_restart_interval,
                       desc.block_size_deviation, len(grandparents),
                       len(survivors))
    for sm, lg, size in grandparents:
        out += _lp(sm) + _lp(lg) + struct.pack("<Q", size)
    for k, v in survivors:
        out += _lp(k) + struct.pack("<I", len(v))
    return bytes(out)


@pytest.fixture(scope="module")
def cut_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not installed")
    exe = tmp_path_factory.mktemp("cut_host") / "cut_host"
    csrc = os.path.join(REPO, "toplingdb_amd", "csrc")
    r = subprocess.run(
        ["g++", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-I", csrc, "-o", str(exe),
         os.path.join(REPO, "tools", "cut_host", "cut_host.cpp"),
         os.path.join(csrc, "dcw_host.cpp"), "-l:libzstd.so.1"],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


def test_cutter_matches_oracle(cut_host, tmp_path):
    fired = dict.fromkeys(RULES, 0)
    gp_mid_block = gp_block_boundary = 0
    for job in jobs():
        assert job.job_kw["compression"] == 0
        out = tmp_path / job.name
        out.mkdir()
        desc = oracle.make_job(job.write_inputs(tmp_path), str(out),
                               **job.kw())
        want = oracle.execute(desc)["files"]
        assert len(want) >= 2, job.name
        if not job.grandparents:
            assert len(want) >= 3, job.name
        survivors = []
        for f in want:
            with open(f["path"], "rb") as fh:
                survivors += oracle.read_sst(fh.read())
        path = tmp_path / (job.name + ".cut")
        path.write_bytes(job_file(desc, job.grandparents, survivors))
        r = subprocess.run([cut_host, str(path)], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, job.name + r.stdout[-2000:] + r.stderr[-3000:]
        lines = r.stdout.split("\n")
        assert lines[-2:] == ["OK", ""], job.name
        got = [ln.split() for ln in lines[:-2]]
        print(job.name, "files:", len(got), "rules:",
              sorted({g[3] for g in got}), "partial_count:",
              sorted({int(g[4]) for g in got[:-1]}))
        assert len(got) == len(want), job.name
        for (tag, first, count, rule, partial), f in zip(got, want):
            first, count, partial = int(first), int(count), int(partial)
            assert tag == "file"
            assert count == f["num_entries"], job.name
            assert survivors[first][0] == f["smallest"], job.name
            assert survivors[first + count - 1][0] == f["largest"], job.name
            if rule == "end":
                continue
            fired[rule] += 1
            if job.grandparents:
                gp_mid_block += partial > 0
                gp_block_boundary += partial == 0
            else:
                assert rule == "size" and partial == 1, job.name
        assert [g[3] for g in got[:-1]].count("end") == 0, job.name
        assert got[-1][3] == "end", job.name
    assert all(fired.values()), fired
    assert gp_mid_block and gp_block_boundary, (gp_mid_block,
                                                gp_block_boundary)
