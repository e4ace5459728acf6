"""The zstd input decoder against libzstd, without a GPU.

tools/zstd_host compiles toplingdb_amd/csrc/dcw_zstd_dec.h, the very source
k_decompress_zstd compiles, under -fsanitize=address,undefined and runs the
wave decoder in the kernel's schedule (lane loops per phase, both lane orders)
on buffers of exactly the kernel's sizes.  Every good frame of
tests/foreign_zstd.py must decode to libzstd's bytes; of the seeded mutations
every one libzstd refuses must be refused, and none may be accepted with
other bytes than libzstd's.  The format-mode counters cover every record the
decoder ran on: a 3-byte sequence count means at least 0x7f00 sequences,
which no frame within DEC_MAX can hold, so that form is counted on a refused
stream.
"""
import os
import shutil
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import foreign_zstd as fz  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """-> (records, the tool's result) for the one corpus."""
    if shutil.which("g++") is None:
        pytest.fail("g++ not installed")
    d = tmp_path_factory.mktemp("zstd_host")
    exe = str(d / "zstd_host")
    r = subprocess.run(
        ["g++", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-I",
         os.path.join(REPO, "toplingdb_amd", "csrc"), "-o", exe,
         os.path.join(REPO, "tools", "zstd_host", "zstd_host.cpp")],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    records = [(name, fz.frame_block(f, len(raw)), raw)
               for name, (f, raw) in fz.good_frames().items()]
    records += [("host_only%d" % i, p, "host")
                for i, p in enumerate(fz.host_only_blocks())]
    records += fz.mutations() + [("nseq_3byte", fz.too_many_sequences(), None)]
    with open(d / "corpus.bin", "wb") as f:
        for name, payload, want in records:
            if want is None or want == "host":
                f.write(struct.pack("<III", len(payload), 0,
                                    0xffffffff if want is None else 0xfffffffe))
                f.write(payload)
            else:
                may_refuse = "." in name  # a mutation libzstd still decodes
                f.write(struct.pack("<III", len(payload),
                                    len(want) | may_refuse << 31, len(want)))
                f.write(payload + want)
    return records, subprocess.run([exe, str(d / "corpus.bin")],
                                   capture_output=True, text=True, timeout=300)


def test_corpus_decodes_as_libzstd(report):
    records, r = report
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stderr == ""  # sanitizer-clean
    lines = r.stdout.split("\n")
    muts = fz.mutations()
    refused = sum(want is None for _, _, want in muts)
    assert 2 * refused >= len(muts) >= 6 * 40
    assert lines[-3:] == [
        "zstd_host: %d records (%d decoded, %d malformed, 2 host-only), "
        "0 failures" % (len(records), len(records) - refused - 3, refused + 1),
        "OK", ""]


def test_every_format_mode_ran(report):
    modes = dict(l.split()[1:] for l in report[1].stdout.split("\n")
                 if l.startswith("mode "))
    assert len(modes) == 33
    assert [m for m, n in modes.items() if int(n) == 0] == []
