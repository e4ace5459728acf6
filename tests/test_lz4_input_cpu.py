"""The LZ4 input decoders against the Python statement of their spec,
without a GPU.

tools/lz4_host compiles toplingdb_amd/csrc/dcw_lz4_dec.h, the very source
that k_decompress_lz4 compiles, as a stand-alone program under
-fsanitize=address,undefined: lz4_dec_lds on buffers of exactly DEC_MAX +
DEC_PAD bytes, lz4_dec on buffers of exactly the stream and the decoded size.
Both must give what tests/foreign_lz4.py `decode` gives on every stream of
the corpus the GPU test decodes, and refuse what it refuses.
"""
import os
import shutil
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import foreign_lz4 as fl  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lz4_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not installed")
    exe = tmp_path_factory.mktemp("lz4_host") / "lz4_host"
    r = subprocess.run(
        ["g++", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-I",
         os.path.join(REPO, "toplingdb_amd", "csrc"), "-o", str(exe),
         os.path.join(REPO, "tools", "lz4_host", "lz4_host.cpp")],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


def test_decoders_match_python_reference(lz4_host, tmp_path):
    good, bad = fl.streams()
    assert fl.directed_stream.ended_on_match > 0  # zero final literals
    assert max(len(raw) for _, raw in good) >= 65536
    path = tmp_path / "corpus.bin"
    on_lds = good_global = 0
    with open(path, "wb") as f:
        for payload, raw in good:
            size, s = fl.unframe(payload)
            assert fl.decode(s, size) == raw
            on_lds += len(s) <= fl.DEC_MAX and size <= fl.DEC_MAX
            good_global += len(s) > fl.DEC_MAX or size > fl.DEC_MAX
            f.write(struct.pack("<III", len(payload), size, len(raw)) +
                    payload + raw)
        for payload in bad:
            with pytest.raises(fl.Lz4Error):
                size, s = fl.unframe(payload)
                on_lds += len(s) <= fl.DEC_MAX and size <= fl.DEC_MAX
                fl.decode(s, size)
            f.write(struct.pack("<III", len(payload), 0, 0xffffffff) + payload)
    # both sides of the LDS/global split, and every malformed stream
    assert on_lds > 100 and good_global >= 3
    assert len(bad) == 2 * len(fl.MALFORMED_NAMES)
    r = subprocess.run([lz4_host, str(path)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stderr == ""  # sanitizer-clean
    assert r.stdout.split("\n")[-3:] == [
        "lz4_host: %d records (%d malformed, %d on the LDS form), 0 failures"
        % (len(good) + len(bad), len(bad), on_lds), "OK", ""]
