"""tools/lz4_enc_host, a stand-alone program under ASan/UBSan, runs
dcw_lz4_enc.h in k_compress_lz4's schedule and checks it against the serial
restatement and lz4_dec; here each payload must equal tests/lz4_out_spec.py."""
import os
import random
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lz4_out_spec as spec  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (13, 17, 100, 4096, 4100, 16384, 16385, 65535, 65536, 65537, 65548,
         200000)
WORDS = [bytes(random.Random(w).choices(range(97, 123), k=3 + w % 7))
         for w in range(30)]
NAMES = ["%s-%d" % (c, n) for c in ("zeros", "mix", "random") for n in SIZES]
DIRECTED = {"seam": spec.seam_block, "match_lengths": spec.match_length_block}


def block(name):
    if name in DIRECTED:
        return DIRECTED[name]()
    content, n = name.split("-")[0], int(name.split("-")[1])
    rng = random.Random(name)
    return {"zeros": bytes(n), "random": rng.randbytes(n),
            "mix": b" ".join(rng.choices(WORDS, k=n // 4 + 1))[:n]}[content]


@pytest.fixture(scope="module")
def payloads(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lz4_enc_host")
    exe, corpus, out = (str(tmp / f) for f in ("tool", "corpus", "streams"))
    subprocess.run(
        ["g++", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-I",
         os.path.join(REPO, "toplingdb_amd", "csrc"), "-o", exe,
         os.path.join(REPO, "tools", "lz4_enc_host", "lz4_enc_host.cpp")],
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
    raw = block(name)
    found = spec.matches(raw)
    assert payloads[name] == spec.frame(spec.emit(raw, found), len(raw))
    size, stream = spec.unframe(payloads[name])
    assert size == len(raw) and spec.decode(stream, size) == raw
    return raw, found


@pytest.mark.parametrize("name", NAMES)
def test_schedule_restatement_and_spec_agree(payloads, name):
    raw, found = check(payloads, name)
    if name.startswith("random"):
        assert not found and spec.encode(raw) is None
    elif len(raw) >= 4096:
        assert spec.encode(raw) == payloads[name]


def test_seam_runs(payloads):
    # literal runs handed on: lengths around the nibble (15) and the first
    # extension byte (270), across 1, 2 and 5 match-less lanes, lane 0 too
    raw, found = check(payloads, "seam")
    assert spec.encode(raw) is not None
    runs, spans, at, lane = set(), set(), 0, -1
    for p, _, ln in found:
        runs.add(p - at)
        spans.add(p // 64 - lane - 1)
        at, lane = p + ln, p // 64
    assert {14, 15, 16, 269, 270, 271} <= runs
    assert {1, 2, 5} <= spans and found[0][0] // 64 == 1


def test_match_lengths(payloads):
    _, found = check(payloads, "match_lengths")
    assert set(spec.MATCH_LENGTHS) <= {ln for _, _, ln in found}
