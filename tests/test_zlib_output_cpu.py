"""tools/zlib_enc_host, a stand-alone program under ASan/UBSan, runs the wave
form of dcw_deflate_enc.h (the text k_compress_zlib compiles) with the lanes
in a loop and checks it against the serial restatement and inflate_dec; here
each payload must equal tests/zlib_out_spec.py and decode with Python's zlib."""
import os
import random
import struct
import subprocess
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import foreign_lz4 as fl  # noqa: E402
import zlib_out_spec as spec  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 3, 17, 100, 4096, 4100, 16383, 16384, 16385, 32769, 70000)
WORDS = [bytes(random.Random(w).choices(range(97, 123), k=3 + w % 7))
         for w in range(30)]
NAMES = ["%s-%d" % (c, n) for c in ("zeros", "mix", "random") for n in SIZES]
DIRECTED = {"boundaries": spec.boundary_block, "three_windows": spec.three_window_block}


def block(name):
    if name in DIRECTED:
        return DIRECTED[name]()
    content, n = name.split("-")[0], int(name.split("-")[1])
    rng = random.Random(name)
    return {"zeros": bytes(n), "random": rng.randbytes(n),
            "mix": b" ".join(rng.choices(WORDS, k=n // 4 + 1))[:n]}[content]


@pytest.fixture(scope="module")
def payloads(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("zlib_enc_host")
    exe, corpus, out = (str(tmp / f) for f in ("tool", "corpus", "streams"))
    subprocess.run(
        ["g++", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-I",
         os.path.join(REPO, "toplingdb_amd", "csrc"), "-o", exe,
         os.path.join(REPO, "tools", "zlib_enc_host", "zlib_enc_host.cpp")],
        check=True)
    names = NAMES + list(DIRECTED)
    with open(corpus, "wb") as f:
        for name in names:
            f.write(struct.pack("<I", len(name)) + name.encode() +
                    struct.pack("<I", len(block(name))) + block(name))
    r = subprocess.run([exe, corpus, out], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("OK\n"), \
        r.stdout[-2000:] + r.stderr[-3000:]
    got, at, streams = {}, 0, open(out, "rb").read()
    for name in names:
        (cn,) = struct.unpack_from("<I", streams, at)
        got[name] = streams[at + 4:at + 4 + cn]
        at += 4 + cn
    assert at == len(streams)
    return got


def check(payloads, name):
    """-> (block, form of each window, whether the ratio rule accepts)"""
    raw = block(name)
    payload, forms, far = spec.stream(raw)
    assert payloads[name] == payload
    size, body = fl.unframe(payload)
    d = zlib.decompressobj(wbits=-14)
    assert size == len(raw) and d.decompress(body) == raw
    assert d.eof and d.unused_data == b""
    assert far <= 16383
    assert forms[0] == {1: "fixed", 2: "dynamic"}[body[0] >> 1 & 3]
    assert body[0] & 1 == (len(raw) <= spec.WINDOW)
    return raw, forms, spec.encode(raw) is not None


@pytest.mark.parametrize("name", NAMES)
def test_tool_spec_and_zlib_agree(payloads, name):
    raw, forms, accepted = check(payloads, name)
    if name.startswith("random") and len(raw) >= 100:
        assert not accepted
    if name in ("zeros-17", "zeros-100"):
        assert forms == ["fixed"] and accepted
    if name in ("mix-4096", "zeros-16384", "mix-70000"):
        assert set(forms) == {"dynamic"} and accepted


def test_boundaries(payloads):
    raw, forms, accepted = check(payloads, "boundaries")
    found = [s for s in spec.window_symbols(raw, 0, len(raw)) if isinstance(s, tuple)]
    assert set(spec.LENGTH_EDGES) <= {ln for ln, _ in found}
    assert set(spec.DISTANCE_EDGES) <= {d for _, d in found}
    assert forms == ["dynamic"]


def test_three_windows(payloads):
    # no distance code, one distance symbol of length 1, then two
    raw, forms, accepted = check(payloads, "three_windows")
    used = [{spec.classify(s[1], spec.DIST_BASE)[0]
             for s in spec.window_symbols(raw, b, min(b + spec.WINDOW, len(raw)))
             if isinstance(s, tuple)} for b in range(0, len(raw), spec.WINDOW)]
    assert [len(u) for u in used] == [0, 1, 2] and forms == ["dynamic"] * 3
    assert accepted


def test_word_text_stores_below_lz4():
    # the issue's condition: Huffman-coded literals must pay for the header
    import foreign_zlib as fz
    import lz4_out_spec as lz4
    rng = random.Random(7)
    for _ in range(8):
        raw = fz.word_text(4096, rng)
        assert len(spec.encode(raw)) < len(lz4.encode(raw))
