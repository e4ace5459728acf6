"""CPU side of the DZT-input tests: the foreign-file helper round-trips
through the oracle reader, the corpus the GPU tests decode covers every op
class the decoder must accept, and tools/dzt_in_host — the kernels' own
decoder sources plus the worker's DZT parser, built with
-fsanitize=address,undefined as a stand-alone program — decodes that corpus,
refuses the malformed list and agrees with the oracle codec under fuzz."""
import os
import shutil
import struct
import subprocess
import sys
from collections import Counter

import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dzt_foreign as zf  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def foreign(tmp_path_factory):
    """(original file bytes, dict, {mode: rewritten file bytes})."""
    path, d = zf.foreign_file(tmp_path_factory.mktemp("zf"))
    data = open(path, "rb").read()
    return data, d, {m: zf.rewrite(data, zf.encoder(m), d) for m in zf.MODES}


def test_parts_rebuild_is_identity(foreign):
    data, _, _ = foreign
    assert zf.Dzt(data).build() == data


def test_rewritten_files_read_back(foreign):
    data, d, files = foreign
    want = oracle.dzt_read(data)
    assert len(want) == 720
    for mode, f in files.items():
        assert f != data
        assert oracle.dzt_read(f) == want, mode
        z = zf.Dzt(f)
        assert z.dict == d
        assert len(z.vblocks) >= 2 and len(z.kblocks) >= 2


def test_corpus_covers_every_op_class(foreign):
    """The GPU foreign-stream test decodes exactly these files; a corpus
    change that drops a class fails here."""
    _, d, files = foreign
    total = Counter()
    for f in files.values():
        z = zf.Dzt(f)
        for btype, body, ulen, _ in z.vblocks:
            if btype == 2:
                total += zf.classify(bytes(body), len(d))
    missing = [c for c in zf.REQUIRED_CLASSES if not total[c]]
    assert not missing, (missing, total)


def test_oracle_encoder_reaches_few_classes(foreign):
    """Why the helper's encoder is needed."""
    data, _, _ = foreign
    z = zf.Dzt(data)
    total = Counter()
    for btype, body, ulen, _ in z.vblocks:
        if btype == 2:
            total += zf.classify(bytes(body), len(z.dict))
    assert total["copy_tag3"] == 0
    assert not any(total["overlap_%d" % k] for k in range(1, 17))


def test_classifier_refuses_malformed_streams(foreign):
    data, _, _ = foreign
    for name in ("copy_offset_0", "copy_offset_beyond_dict", "output_overrun",
                 "truncated_op", "literal_len_near_2_32"):
        z = zf.Dzt(zf.malformed(data, name))
        with pytest.raises(zf.StreamError):
            zf.classify(bytes(z.vblocks[0][1]), len(z.dict))
        with pytest.raises(ValueError):
            oracle.snappy_uncompress_dict(z.dict, bytes(z.vblocks[0][1]))


# what refuses each malformed file: the host parser, or a decoder/kernel
HOST_REFUSED = {"records_65", "first_rank_not_monotone",
                "koff_ksize_past_key_area", "flip_key_area", "flip_dict"}
STREAM_REFUSED = {"copy_offset_0", "copy_offset_beyond_dict", "output_overrun",
                  "truncated_op", "literal_len_near_2_32"}
KEYBLOCK_REFUSED = {"shared_gt_U", "shared_plus_nonshared_ne_U",
                    "value_type_merge", "records_out_of_order"}


def _rec(kind, a, b, c, *payload):
    return kind + struct.pack("<3I", a, b, c) + b"".join(payload)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_host_tool_sanitized(tmp_path, foreign):
    data, d, files = foreign
    exe = tmp_path / "dzt_in_host"
    orc = os.path.join(REPO, "oracle")
    csrc = os.path.join(REPO, "toplingdb_amd", "csrc")
    r = subprocess.run(
        ["g++", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-I", csrc, "-o", str(exe),
         os.path.join(REPO, "tools", "dzt_in_host", "dzt_in_host.cpp"),
         os.path.join(csrc, "dcw_host.cpp"),
         os.path.join(orc, "liborc.so"), "-l:libzstd.so.1",
         "-Wl,-rpath," + orc],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    corpus = bytearray()
    ns = nk = nf = nrej = 0
    for f in list(files.values()) + [data]:
        z = zf.Dzt(f)
        corpus += _rec(b"F", len(f), 1, 0, f)
        nf += 1
        for i, (btype, body, ulen, _) in enumerate(z.vblocks):
            if btype != 2:
                continue
            raw = z.raw_block(i)
            assert len(raw) == ulen
            corpus += _rec(b"S", len(z.dict), len(body), ulen, z.dict,
                           bytes(body), raw)
            ns += 1
    z = zf.Dzt(data)
    for kb, (_, koff, ksize, _) in enumerate(z.kblocks):
        recs = zf._records(z, kb)
        want = b"".join(k + struct.pack("<QII", t, vo, vl)
                        for k, t, vo, vl in recs)
        corpus += _rec(b"K", z.U, ksize, len(recs),
                       bytes(z.key_area[koff:koff + ksize]), want)
        nk += 1
    for name in zf.MALFORMED:
        bad = zf.malformed(data, name)
        host = name in HOST_REFUSED
        corpus += _rec(b"F", len(bad), 0 if host else 1, 0, bad)
        nf += 1
        nrej += host
        if host or name.startswith("flip_"):
            continue
        zb = zf.Dzt(bad)
        if name in STREAM_REFUSED:
            corpus += _rec(b"S", len(zb.dict), len(zb.vblocks[0][1]),
                           0xFFFFFFFF, zb.dict, bytes(zb.vblocks[0][1]))
            ns += 1
            nrej += 1
        if name in KEYBLOCK_REFUSED:
            _, koff, ksize, _ = zb.kblocks[-1]
            corpus += _rec(b"K", zb.U, ksize, 0xFFFFFFFF,
                           bytes(zb.key_area[koff:koff + ksize]))
            nk += 1
            nrej += 1
    path = tmp_path / "corpus.bin"
    path.write_bytes(bytes(corpus))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "corpus: %d streams, %d key blocks, %d files (%d refused)" % (
        ns, nk, nf, nrej) in r.stdout
    assert "fuzz: 3000 streams" in r.stdout
    assert r.stdout.rstrip().endswith("OK")
