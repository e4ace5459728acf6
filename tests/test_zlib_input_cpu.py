"""The zlib input decoders of dcw_inflate_dec.h, the source k_decompress_zlib
compiles, against Python's zlib: tools/zlib_host under ASan/UBSan over every
stream of tests/foreign_zlib.py, into buffers of exactly the promised size."""
import os
import re
import shutil
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import foreign_zlib as fz  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def zlib_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not installed")
    exe = tmp_path_factory.mktemp("zlib_host") / "zlib_host"
    r = subprocess.run(
        ["g++", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-I",
         os.path.join(REPO, "toplingdb_amd", "csrc"), "-o", str(exe),
         os.path.join(REPO, "tools", "zlib_host", "zlib_host.cpp")],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


def test_decoders_match_zlib(zlib_host, tmp_path):
    recs = fz.streams()
    flips = fz.flips()
    # zlib alone refuses a good share of the flips: the corpus has teeth
    assert len(flips) >= 200 and sum(w is None for _, _, w in flips) >= len(flips) // 4
    for name, (s, size) in fz.malformed(fz.word_text(3000, fz.random.Random(1))).items():
        assert fz.verdict(s, size) is None, name
    path = tmp_path / "corpus.bin"
    with open(path, "wb") as f:
        for s, size, want in recs:
            assert fz.verdict(s, size) == want
            f.write(struct.pack("<III", len(s), size, 0xffffffff if want is None else size) +
                    s + (want or b""))
    good = sum(w is not None for _, _, w in recs)
    assert max(size for _, size, w in recs if w is not None) >= 200000
    r = subprocess.run([zlib_host, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stderr == ""  # sanitizer-clean
    lines = r.stdout.split("\n")
    assert lines[-2:] == ["OK", ""]
    m = re.fullmatch(
        r"zlib_host: (\d+) records \((\d+) decoded, (\d+) refused\), blocks: (\d+) stored, "
        r"(\d+) fixed \((\d+) table builds\), (\d+) dynamic; longest code (\d+); most match "
        r"rounds (\d+); 0 failures", lines[-3])
    assert m, lines[-3]
    n, decoded, refused, stored, fixed, builds, dynamic, longest, rounds = map(int, m.groups())
    assert (n, decoded, refused) == (len(recs), good, len(recs) - good)
    assert stored > 0 and dynamic > 0 and 0 < builds < fixed  # a run of fixed blocks builds once
    assert longest == 15
    assert rounds > 1
