"""The large-frame zstd input decoder against libzstd, without a GPU.

tools/zstd_large_host compiles toplingdb_amd/csrc/dcw_zstd_dec_large.h, the
very source k_decompress_zstd_large compiles, under
-fsanitize=address,undefined and runs the wave decoder in the kernel's
schedule (lane loops per phase, both lane orders) on buffers of exactly the
sizes the kernel may touch.  Every frame of large_frames() must decode to
libzstd's bytes; of the seeded single-byte flips every one libzstd refuses
must be refused, and none may be accepted with other bytes than libzstd's.
"""
import os
import random
import shutil
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import foreign_zstd as fz  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _far_repeat(rng):
    """300000 bytes, three blocks; 50000 random bytes come again about 200000
    bytes later, so one offset crosses two block borders"""
    a = rng.randbytes(50000)
    return a + fz._record_text(150000, rng) + a + fz._record_text(50000, rng)


def _tokens(rng):
    """128 KiB of 3-byte tokens, each followed by one fresh byte"""
    toks = [rng.randbytes(3) for _ in range(40)]
    return b"".join(rng.choice(toks) + rng.randbytes(1) for _ in range(32768))


def _seq_section_first_byte(frame):
    """first byte of the sequences section of the frame's first block"""
    fhd = frame[4]
    single = fhd >> 5 & 1
    at = 5 + (not single) + (single, 2, 4, 8)[fhd >> 6]
    if frame[at] >> 1 & 3 != 2:
        return None
    at += 3
    kind, sf = frame[at] & 3, frame[at] >> 2 & 3
    word = int.from_bytes(frame[at:at + 5], "little")
    if kind < 2:
        lh = (1, 2, 1, 3)[sf]
        size = word >> 3 & 31 if lh == 1 else word >> 4 & (0xfff if lh == 2 else 0xfffff)
        return frame[at + lh + (size if kind == 0 else 1)]
    lh, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
    return frame[at + lh + (word >> 4 + bits & (1 << bits) - 1)]


def nseq3_frame(rng):
    """-> (frame, raw) with a block whose sequence count takes 3 bytes"""
    raw = _tokens(rng)
    frame = fz.compress(raw, 19)
    if _seq_section_first_byte(frame) == 255:
        return frame, raw
    n = 0x7f00 + 70
    seqs = [(rng.randrange(4), 0, 0) for _ in range(n)]
    frame = fz.hand_frame([fz.raw_block(b"head"), fz.seq_block(
        rng.randbytes(n + 3), (1, 2, 1), seqs, True, nseq_form=3)], 5 * n + 7, 4)
    return frame, fz.decompress(frame, 5 * n + 7)


# name -> (content, compress() arguments)
CASES = {
    "text_4993": (lambda r: fz._record_text(4993, r), {}),
    "zeros_100000": (lambda r: bytes(100000), {}),
    "text_16384_l1": (lambda r: fz._record_text(16384, r), dict(level=1)),
    "text_65536_l19": (lambda r: fz._record_text(65536, r), dict(level=19)),
    "text_131072": (lambda r: fz._record_text(131072, r), {}),
    "text_131073": (lambda r: fz._record_text(131073, r), {}),
    "far_repeat_300000": (_far_repeat, {}),
    "far_repeat_l19": (_far_repeat, dict(level=19)),
    "skewed_65536": (lambda r: fz._skewed(65536, r, 256), {}),
    "skewed_16384_l19": (lambda r: fz._skewed(16384, r, 256), dict(level=19)),
    "random_300000": (lambda r: r.randbytes(300000), dict(level=1)),
    "flushed_65536": (lambda r: fz._record_text(65536, r),
                      dict(flush_at=tuple(range(2500, 65536, 2500)))),
    "flushed_skewed": (lambda r: fz._skewed(40000, r, 256),
                       dict(level=19, flush_at=tuple(range(6000, 40000, 6000)))),
}
MUTATED = ("text_16384_l1", "skewed_65536", "far_repeat_300000")


def large_frames():
    rng = random.Random(0x1A46E)
    out = {}
    for name, (make, kw) in CASES.items():
        raw = make(rng)
        out[name] = (fz.compress(raw, **kw), raw)
    out["nseq_3byte"] = nseq3_frame(rng)
    return out


def mutations(frames, per_frame=20):
    """-> [(name, stored block, libzstd's bytes or None)]"""
    rng = random.Random(0xF11B)
    out = []
    for name in MUTATED:
        frame, raw = frames[name]
        for k in range(per_frame):
            at = k if k < 8 else rng.randrange(8, len(frame))
            m = bytearray(frame)
            m[at] ^= 1 << rng.randrange(8)
            out.append(("%s.flip@%d" % (name, at), fz.frame_block(bytes(m), len(raw)),
                        fz.decompress(bytes(m), len(raw))))
    return out


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """-> (frames, mutations, the tool's result) for the one corpus."""
    if shutil.which("g++") is None:
        pytest.fail("g++ not installed")
    d = tmp_path_factory.mktemp("zstd_large_host")
    exe = str(d / "zstd_large_host")
    r = subprocess.run(
        ["g++", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-I",
         os.path.join(REPO, "toplingdb_amd", "csrc"), "-o", exe,
         os.path.join(REPO, "tools", "zstd_large_host", "zstd_large_host.cpp")],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    frames = large_frames()
    muts = mutations(frames)
    with open(d / "corpus.bin", "wb") as f:
        for name, (frame, raw) in frames.items():
            assert fz.decompress(frame, len(raw)) == raw, name
            payload = fz.frame_block(frame, len(raw))
            f.write(struct.pack("<III", len(payload), len(raw), len(raw)) + payload + raw)
        for name, payload, want in muts:
            if want is None:
                f.write(struct.pack("<III", len(payload), 0, 0xffffffff) + payload)
            else:
                f.write(struct.pack("<III", len(payload), len(want) | 1 << 31,
                                    len(want)) + payload + want)
    return frames, muts, subprocess.run([exe, str(d / "corpus.bin")],
                                        capture_output=True, text=True, timeout=300)


def test_corpus_decodes_as_libzstd(report):
    frames, muts, r = report
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stderr == ""  # sanitizer-clean
    refused = sum(want is None for _, _, want in muts)
    assert len(muts) == 60 and refused >= 20
    lines = r.stdout.split("\n")
    assert lines[-2:] == ["OK", ""]
    assert lines[-3].startswith("zstd_large_host: %d records" % (len(frames) + 60))
    assert ", %d malformed, " % refused in lines[-3]
    # every good frame was decoded in both orders; the 3-byte count ran
    assert int(lines[-3].split("(")[1].split()[0]) >= len(frames)
    assert " 0 with a 3-byte" not in lines[-3]
