"""zstd frames from outside the project: libzstd (ctypes) makes and judges
them; a few frames that libzstd does not emit at these sizes are assembled by
hand (RLE-mode sequence tables carry no state bits, so a sequence is its extra
bits alone) and checked with ZSTD_decompress before use.  A stored block of
type 7 is `frame_block(frame, size)`: varint32(size) + frame.
"""
import ctypes
import functools
import random

from foreign_lz4 import frame as frame_block  # varint32(size) + frame

ZSTD = 7
DEC_MAX = 4992  # dcw_zstd_dec.h kZstdMax
_lib = ctypes.CDLL("libzstd.so.1")
for _f in ("ZSTD_compress2", "ZSTD_decompress", "ZSTD_compressStream2",
           "ZSTD_CCtx_setParameter", "ZSTD_freeCCtx"):
    getattr(_lib, _f).restype = ctypes.c_size_t
_lib.ZSTD_createCCtx.restype = ctypes.c_void_p
_lib.ZSTD_isError.argtypes = [ctypes.c_size_t]


class _Buf(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("size", ctypes.c_size_t),
                ("pos", ctypes.c_size_t)]


def decompress(frame, size):
    """libzstd's verdict as the worker takes it: the bytes, or None unless
    exactly `size` bytes come out."""
    dst = ctypes.create_string_buffer(max(size, 1))
    got = _lib.ZSTD_decompress(dst, size, bytes(frame), len(frame))
    if _lib.ZSTD_isError(got) or got != size:
        return None
    return dst.raw[:size]


def compress(raw, level=3, checksum=False, flush_at=()):
    """One frame.  flush_at: input positions of ZSTD_e_flush (a block ends
    there; such frames carry no content size)."""
    c = ctypes.c_void_p(_lib.ZSTD_createCCtx())
    for param, v in ((100, level), (201, int(checksum))):
        assert not _lib.ZSTD_isError(_lib.ZSTD_CCtx_setParameter(
            c, ctypes.c_int(param), ctypes.c_int(v)))
    cap = len(raw) + 1024
    dst = ctypes.create_string_buffer(cap)
    if not flush_at:
        got = _lib.ZSTD_compress2(c, dst, ctypes.c_size_t(cap), raw,
                                  ctypes.c_size_t(len(raw)))
        assert not _lib.ZSTD_isError(got)
    else:
        src = ctypes.create_string_buffer(raw, max(len(raw), 1))
        ob = _Buf(ctypes.addressof(dst), cap, 0)
        ib = _Buf(ctypes.addressof(src), 0, 0)
        for end, op in [(e, 1) for e in flush_at] + [(len(raw), 2)]:
            ib.size = end
            while True:
                left = _lib.ZSTD_compressStream2(
                    c, ctypes.byref(ob), ctypes.byref(ib), ctypes.c_int(op))
                assert not _lib.ZSTD_isError(left)
                if left == 0:
                    break
        got = ob.pos
    _lib.ZSTD_freeCCtx(c)
    return dst.raw[:got]


# ------------------------------------------------------------- hand assembly
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13,
                      14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12,
                      13, 14, 15, 16]


def _block(kind, body, last, size=None):
    h = (len(body) if size is None else size) << 3 | kind << 1 | int(last)
    return h.to_bytes(3, "little") + body


def raw_block(data, last=False):
    return _block(0, data, last)


def rle_block(byte, n, last=False):
    return _block(1, bytes([byte]), last, n)


def seq_block(literals, syms, seqs, last=False, nseq_form=None, repeat=False):
    """Compressed block, raw literals, all three tables in RLE mode with the
    codes syms = (ll, of, ml); seqs = [(offset bits, ml bits, ll bits)], the
    extra-bit values of each sequence.  repeat: all three in repeat mode,
    syms being the codes the tables in place hold."""
    rle = isinstance(literals, tuple)  # (byte, count): RLE literals
    n = literals[1] if rle else len(literals)
    lit = ((n << 4 | 0x0c | rle).to_bytes(3, "little") if n > 31
           else bytes([n << 3 | rle])) + (bytes(literals[:1]) if rle else literals)
    widths = (syms[1], ML_BITS[syms[2]], LL_BITS[syms[0]])
    acc = 1
    for s in seqs:
        for v, nb in zip(s, widths):
            assert 0 <= v < 1 << nb
            acc = acc << nb | v
    count = len(seqs)
    form = nseq_form or (1 if count < 128 else 2)
    head = (bytes([count]) if form == 1 else
            bytes([0x80 | count >> 8, count & 255]) if form == 2 else
            bytes([255]) + (count - 0x7f00).to_bytes(2, "little"))
    body = lit + head
    if count:
        body += (b"\xfc" if repeat else bytes([0x54, *syms])) + acc.to_bytes(
            (acc.bit_length() + 7) // 8, "little")
    return _block(2, body, last)


def hand_frame(blocks, size, fcs_bytes=None):
    """Single-segment frame with a content size field of 1, 2, 4 or 8
    bytes."""
    fb = fcs_bytes or (1 if size < 256 else 2)
    v = size - 256 if fb == 2 else size
    return (bytes([0x28, 0xb5, 0x2f, 0xfd, 0x20 | (0, 0, 1, 0, 2, 0, 0, 0, 3)[fb] << 6])
            + v.to_bytes(fb, "little") + b"".join(blocks))


def count_frame(n, fcs_bytes=None):
    """n sequences of 1 literal + a match of 4 at offset 1..4 (hand-made: the
    exact sequence counts around the batch of 64)."""
    rng = random.Random(n)
    seqs = [(rng.randrange(4), 0, 0) for _ in range(n)]
    return hand_frame([raw_block(b"head", False),
                       seq_block(rng.randbytes(n + 3), (1, 2, 1), seqs, True)],
                      4 + 5 * n + 3, fcs_bytes)


def repeat_frame(ll0):
    """Hand-made: repeat-offset values 1, 2, 3 with literal length 0 or 1
    (offset code 0, then code 1 with one extra bit); a last block in repeat
    mode."""
    rng = random.Random(7 + ll0)
    ll = 0 if ll0 else 1
    a = [(0, 0, 0)] * 3
    b = [(0, 0, 0), (1, 0, 0), (1, 0, 0), (0, 0, 0), (1, 0, 0)]
    size = 24 + (len(a) + len(b) + 1) * (ll + 4) + 2
    return hand_frame([raw_block(rng.randbytes(24)),
                       seq_block(rng.randbytes(ll * len(a)), (ll, 0, 1), a),
                       seq_block(rng.randbytes(ll * len(b) + 2), (ll, 1, 1), b),
                       seq_block(rng.randbytes(ll), (ll, 1, 1), b[:1], True,
                                 repeat=True)], size)


# ------------------------------------------------------------------ the corpus
def _skewed(n, rng, symbols=200):
    """geometric byte distribution: a deep Huffman tree"""
    return bytes(min(int(rng.expovariate(0.12)), symbols - 1) for _ in range(n))


def _few(n, rng):
    """20 symbols of small value: libzstd writes their weights directly"""
    return bytes(min(int(rng.expovariate(0.3)), 19) for _ in range(n))


def _matches(rng, specs):
    """random text with, for each (offset, length), a match of that shape"""
    out = bytearray(rng.randbytes(40))
    for off, ln in specs:
        out += rng.randbytes(5)
        for _ in range(ln):
            out.append(out[-off])
    return bytes(out + rng.randbytes(6))


def _record_text(n, rng):
    out = bytearray()
    while len(out) < n:
        out += b"key%06d:value=%s;" % (rng.randrange(3000),
                                       rng.choice([b"alpha", b"beta", b"gamma"]))
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def good_frames():
    """name -> (frame, decoded bytes); every frame decodes with libzstd."""
    rng = random.Random(0x25D)
    out = {}

    def lib(name, raw, **kw):
        out[name] = (compress(raw, **kw), raw)

    def hand(name, frame, size):
        raw = decompress(frame, size)
        assert raw is not None, name
        out[name] = (frame, raw)

    lib("empty", b"")
    lib("one_byte", b"x")
    lib("huf_255", _skewed(255, rng))  # one Huffman stream
    lib("huf_256", _skewed(256, rng))  # four
    lib("rle_block", b"\x07" * 3000)
    lib("incompressible", rng.randbytes(1500))
    lib("skewed_deep_tree", _skewed(4000, rng), level=19)
    lib("few_symbols", _few(1200, rng))
    lib("short_offsets", _matches(rng, [(o, o * 3 + 5) for o in (1, 2, 3, 7, 8)]),
        level=19)
    lib("long_match", rng.randbytes(300) + b"ab" * 2000 + rng.randbytes(20))
    lib("extra_bits", _matches(rng, [(30, 70), (9, 300), (35, 1100)]) +
        rng.randbytes(700) + _matches(rng, [(20, 40)]), level=19)
    for lvl in (1, 3, 19):
        lib("records_l%d" % lvl, _record_text(4000, rng), level=lvl)
    for size in (DEC_MAX - 1, DEC_MAX):
        lib("size_%d" % size, _record_text(size, rng))
    text = _record_text(4500, rng)
    lib("two_blocks", text, flush_at=(2000,))
    lib("three_blocks", text, level=19, flush_at=(1500, 3000))
    lib("skewed_two_blocks", _skewed(3000, rng, 60), flush_at=(1500,))
    for n in (0, 1, 63, 64, 65, 127, 128):
        size = 4 + 5 * n + 3
        hand("count_%d" % n, count_frame(n, {63: 4, 64: 8}.get(n)), size)
    for ll0 in (0, 1):
        f = repeat_frame(ll0)
        hand("repeat_ll0_%d" % ll0, f, int.from_bytes(f[5:6], "little"))
    hand("rle_literals", hand_frame(
        [raw_block(b"head"), seq_block((0x41, 40), (2, 2, 1),
                                       [(i % 4, 0, 0) for i in range(20)], True)],
        4 + 40 + 80), 124)
    hand("rle_and_raw_blocks", hand_frame(
        [rle_block(9, 300), raw_block(b"tail", True)], 304), 304)
    return out


def host_only_blocks():
    """stored blocks the eligibility walk must leave to the host"""
    rng = random.Random(0x40)
    big = _record_text(DEC_MAX + 1, rng)
    small = _record_text(900, rng)
    return [frame_block(compress(big), len(big)),
            frame_block(compress(small, checksum=True), len(small))]


MUTATED = ("records_l3", "skewed_deep_tree", "three_blocks", "extra_bits",
           "few_symbols", "count_65")


@functools.lru_cache(maxsize=None)
def mutations(seed=0x5EED):
    """-> [(name, stored block, libzstd's bytes or None)]: seeded single-byte
    changes across each frame, truncations, one appended byte."""
    rng = random.Random(seed)
    out = []
    for name in MUTATED:
        frame, raw = good_frames()[name]
        n = len(frame)
        variants = []
        for k in range(36):  # spread over the frame, dense in its first bytes
            at = k if k < 12 else rng.randrange(12, n)
            m = bytearray(frame)
            m[at] ^= 1 << rng.randrange(8) if k % 3 else rng.randrange(1, 256)
            variants.append(("flip%d@%d" % (k, at), bytes(m)))
        variants += [("cut%d" % c, frame[:n - c]) for c in (1, 2, 7, n // 2)]
        variants.append(("append", frame + b"\x00"))
        for tag, m in variants:
            out.append((name + "." + tag, frame_block(m, len(raw)),
                        decompress(m, len(raw))))
    return out


def too_many_sequences():
    """3-byte sequence count (0x7f00 and up cannot fit DEC_MAX: refused)"""
    seqs = [(0, 0, 0)] * 0x7f00
    return frame_block(hand_frame(
        [raw_block(b"head"), seq_block(b"", (0, 0, 1), seqs, True)], 4000), 4000)
