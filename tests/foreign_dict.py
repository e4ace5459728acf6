"""Preset dictionaries from outside the project: libzstd (ctypes) trains them,
compresses with them and judges every frame; lz4_emit writes LZ4 streams with
offsets into one; add_dict_block() gives a file of the oracle's builder a
"rocksdb.compression_dict" meta block."""
import ctypes
import functools
import random

import foreign_corpus as fc
import foreign_lz4 as fl
import foreign_zstd as fz
import oracle

_lib = fz._lib
for _f in ("ZDICT_trainFromBuffer", "ZSTD_compress_usingDict", "ZSTD_CCtx_loadDictionary",
           "ZSTD_decompress_usingDict", "ZSTD_freeDCtx"):
    getattr(_lib, _f).restype = ctypes.c_size_t
_lib.ZSTD_createDCtx.restype = ctypes.c_void_p


@functools.lru_cache(maxsize=None)
def trained(capacity):
    """ZDICT_trainFromBuffer over 300 record-text blocks of 4096 bytes"""
    rng = random.Random(0xD1C7)
    samples = b"".join(fz._record_text(4096, rng) for _ in range(300))
    sizes = (ctypes.c_size_t * 300)(*[4096] * 300)
    dst = ctypes.create_string_buffer(capacity)
    got = _lib.ZDICT_trainFromBuffer(dst, ctypes.c_size_t(capacity), samples, sizes,
                                     ctypes.c_uint(300))
    assert not _lib.ZSTD_isError(got)
    return dst.raw[:got]


def compress(raw, dic, level=3, flush_at=()):
    """One frame coded against `dic`; flush_at as foreign_zstd.compress."""
    c = ctypes.c_void_p(_lib.ZSTD_createCCtx())
    cap = len(raw) + 1024
    dst = ctypes.create_string_buffer(cap)
    if not flush_at:
        got = _lib.ZSTD_compress_usingDict(c, dst, ctypes.c_size_t(cap), raw,
                                           ctypes.c_size_t(len(raw)), dic,
                                           ctypes.c_size_t(len(dic)), ctypes.c_int(level))
        assert not _lib.ZSTD_isError(got)
    else:
        assert not _lib.ZSTD_isError(_lib.ZSTD_CCtx_setParameter(
            c, ctypes.c_int(100), ctypes.c_int(level)))
        assert not _lib.ZSTD_isError(_lib.ZSTD_CCtx_loadDictionary(
            c, dic, ctypes.c_size_t(len(dic))))
        src = ctypes.create_string_buffer(raw, max(len(raw), 1))
        ob = fz._Buf(ctypes.addressof(dst), cap, 0)
        ib = fz._Buf(ctypes.addressof(src), 0, 0)
        for end, op in [(e, 1) for e in flush_at if e < len(raw)] + [(len(raw), 2)]:
            ib.size = end
            while _lib.ZSTD_compressStream2(c, ctypes.byref(ob), ctypes.byref(ib),
                                            ctypes.c_int(op)):
                pass
        got = ob.pos
    _lib.ZSTD_freeCCtx(c)
    return dst.raw[:got]


def decompress(frame, size, dic):
    """ZSTD_decompress_usingDict's verdict: the bytes, or None"""
    d = ctypes.c_void_p(_lib.ZSTD_createDCtx())
    dst = ctypes.create_string_buffer(max(size, 1))
    got = _lib.ZSTD_decompress_usingDict(d, dst, ctypes.c_size_t(size), bytes(frame),
                                         ctypes.c_size_t(len(frame)), dic,
                                         ctypes.c_size_t(len(dic)))
    _lib.ZSTD_freeDCtx(d)
    return None if _lib.ZSTD_isError(got) or got != size else dst.raw[:size]


def frame_info(frame):
    """-> (Dictionary_ID, literals type of the first block or None)"""
    fhd, single, dl = frame[4], frame[4] >> 5 & 1, (0, 1, 2, 4)[frame[4] & 3]
    at = 5 + (not single)
    did = int.from_bytes(frame[at:at + dl], "little")
    at += dl + (single, 2, 4, 8)[fhd >> 6]
    return did, frame[at + 3] & 3 if frame[at] >> 1 & 3 == 2 else None


def lz4_emit(raw, matches, dic):
    """foreign_lz4.emit with offsets that may reach into `dic`"""
    out, at, hist = bytearray(), 0, dic + raw
    for pos, off, ml in matches:
        src = len(dic) + pos - off
        assert at <= pos and 1 <= off <= 65535 and src >= 0 and ml >= 4 and all(
            hist[src + i] == raw[pos + i] for i in range(ml))
        ll = pos - at
        out.append(min(ll, 15) << 4 | min(ml - 4, 15))
        if ll >= 15:
            fl._length(out, ll - 15)
        out += raw[at:pos] + bytes((off & 255, off >> 8))
        if ml - 4 >= 15:
            fl._length(out, ml - 19)
        at = pos + ml
    return bytes(out) + fl.emit(raw[at:], [])  # the last literals


def add_dict_block(sst, dic):
    """The file with `dic` as its "rocksdb.compression_dict" block: cut at the
    metaindex, append the dictionary raw with a trailer, a metaindex that also
    names it, and a footer with the old index handle."""
    foot, vals, rest = sst[-53:], [], sst[-52:]
    for _ in range(4):  # metaindex offset, size; index offset, size
        v, rest = fl.unframe(rest)
        vals.append(v)
    assert vals[2] < vals[0]  # the index block lies before the cut
    meta = sst[vals[0]:vals[0] + vals[1]]
    nrestarts = int.from_bytes(meta[-4:], "little")
    entries, at = [], 0
    while at < len(meta) - 4 - 4 * nrestarts:  # restart interval 1: shared == 0
        assert meta[at] == 0
        ns, vl = meta[at + 1], meta[at + 2]
        entries.append((meta[at + 3:at + 3 + ns], meta[at + 3 + ns:at + 3 + ns + vl]))
        at += 3 + ns + vl
    head = sst[:vals[0]]
    handle = fl.put_varint32(len(head)) + fl.put_varint32(len(dic))

    def block(b):
        return b + b"\0" + oracle.block_checksum(foot[0], b, 0).to_bytes(4, "little")

    body, restarts = b"", []
    for k, v in sorted(entries + [(b"rocksdb.compression_dict", handle)]):
        restarts.append(len(body))
        body += bytes([0, len(k), len(v)]) + k + v
    body += b"".join(r.to_bytes(4, "little") for r in restarts + [len(restarts)])
    head += block(dic)
    handles = b"".join(map(fl.put_varint32, [len(head), len(body)] + vals[2:]))
    return head + block(body) + foot[:1] + handles.ljust(40, b"\0") + foot[41:]


# ------------------------------------------------------------------ the corpus
def periodic_entry(vlen, rng):
    """-> (P, an entry that sorts first and makes its block start with five
    periods of the 8 bytes P: entry header, key, tag and value play along).
    A first match of 40 at offset 8 out of a dictionary that ends in P then
    straddles the border and overlaps itself."""
    p = bytes([0, 23, 0x80 | vlen & 0x7f, 1]) + b"a000"
    seq = int.from_bytes(p[4:] + p[:3], "little")
    return p, (b"a000" + p + p[:3], seq, fc.TYPE_VALUE,
               (p * 3)[3:16] + rng.randbytes(vlen - 13))


def text_kvs(sizes, rng, base=0):
    return [(fc.ukey(base + 2 * i), 1 + i, fc.TYPE_VALUE, fz._record_text(n, rng))
            for i, n in enumerate(sizes)]


def newer_run(n, rng):
    kvs = [(fc.ukey(3 * i), 50000 + i, int(i % 4 != 0),
            b"" if i % 4 == 0 else b"newer-%d" % i * 5) for i in range(n)]
    return fl.build_pair(kvs, lambda i, raw: None, block_size=4096)


def dict_run(kvs, dic, choose, **opts):
    kvs, sst, twin, stored = fl.build_pair(sorted(kvs), choose, **opts)
    return kvs, add_dict_block(sst, dic), twin, stored, dic


def zstd_choose(dic, level=3, first=None, **kw):
    """every block by libzstd against dic; block 0 by first(raw) if given"""
    def choose(i, raw):
        frame = first(raw) if first and i == 0 else compress(raw, dic, level, **kw)
        assert decompress(frame, len(raw), dic) == raw
        return fz.ZSTD, frame
    return choose


def straddle_frame(raw):
    """first sequence: ll 0, ml 40 (code 34 + 1), offset 8 (code 3 + 3)"""
    return fz.hand_frame([fz.seq_block(raw[40:], (0, 3, 34), [(3, 1, 0)], True)], len(raw))


def reach_frame(raw, extra=0, at=0):
    """first sequence: ll 0, ml 8, offset at + 61 + extra from output byte `at`
    (a raw block holds what lies before): with a 61-byte dictionary exactly
    its first byte (extra 1: one before it)"""
    v = at + 64 + extra
    c = v.bit_length() - 1
    return fz.hand_frame([fz.raw_block(raw[:at])] * bool(at) + [fz.seq_block(
        raw[at + 8:], (0, c, 5), [(v - (1 << c), 0, 0)], True)], len(raw), 4 if at else None)


@functools.lru_cache(maxsize=None)
def zstd_job(name):
    rng = random.Random(0x2D + ZSTD_CASES.index(name))
    p, first = periodic_entry(200, rng)
    fill, t4, t16 = rng.randbytes(53), trained(4096), trained(16384)
    small, big = text_kvs([3900, 250] * 40, rng), text_kvs([59900] * 3 + [3000] * 60, rng)
    x = rng.randbytes(8)  # at byte 30000 of the first big value
    marked = [big[0][:3] + (big[0][3][:30000] + x + big[0][3][30008:],)] + big[1:]
    dic, kvs, kw, bs = {
        "trained_4k": (t4, small, {}, 64),
        "trained_1k": (trained(1024), small, {}, 64),
        "raw_content": (t4[200:], small, {}, 64),
        "hand_straddle": (fill + p, [first] + small, dict(first=straddle_frame), 64),
        "hand_first_byte": (p + fill, [first] + small, dict(first=reach_frame), 64),
        "large_60000": (t16, big, {}, 4096),
        "large_two_blocks": (t16, big, dict(flush_at=(30000,)), 32768),
        "large_hand_second_block": (x + fill, marked, dict(
            first=lambda raw: reach_frame(raw, at=raw.find(x))), 4096)}[name]
    return [dict_run(kvs, dic, zstd_choose(dic, **kw), block_size=bs),
            newer_run(30, rng) + (None,)]


ZSTD_CASES = ("trained_4k", "trained_1k", "raw_content", "hand_straddle", "hand_first_byte",
              "large_60000", "large_two_blocks", "large_hand_second_block")


@functools.lru_cache(maxsize=None)
def lz4_job(name, btype=fl.LZ4):
    """Block 0 of run 0: a straddling, self-overlapping match at its first byte,
    then one wholly inside the dictionary at the largest offset that reaches
    it (4 KiB: the dictionary's first byte)."""
    rng = random.Random(0x4D + sorted(LZ4_CASES).index(name))
    size, big = LZ4_CASES[name]
    p, first = periodic_entry(200, rng)
    reach = min(size, 65535)
    far = min(40 + reach, 65535)  # the second match's offset, from block byte 40
    tail = bytearray(rng.randbytes(reach - 8) + p)
    tail[reach + 40 - far:reach + 56 - far] = first[3][13:29]  # block bytes 40..56
    dic = rng.randbytes(size - reach) + bytes(tail)
    kvs = [first] + text_kvs([6000 if big else 300] + [300] * 150, rng)

    def choose(i, raw):
        return btype, (lz4_emit(raw, [(0, 8, 40), (40, far, 16)], dic)
                       if i == 0 else fl.best(raw))

    return [dict_run(kvs, dic, choose, block_size=8192 if big else 1024),
            newer_run(30, rng) + (None,)]


LZ4_CASES = {"dict_4k": (4096, False), "dict_70000": (70000, False),
             "block_over_dec_max": (4096, True)}


def refusals():
    """name -> (dictionary, stored type, payload, libzstd's verdict or None)"""
    rng = random.Random(0xBAD)
    raw = fz._record_text(3000, rng)
    d4 = trained(4096)
    good = compress(raw, d4)
    did = bytearray(good)
    did[5 + (not good[4] >> 5 & 1)] ^= 1  # first byte of the Dictionary_ID
    cut = d4[:60]  # full dictionary, its entropy section cut short
    short = rng.randbytes(61)
    past = reach_frame(short[:8] + raw, extra=1)
    out = {"wrong_dict_id": (d4, fz.ZSTD, bytes(did), len(raw)),
           "zstd_offset_past_dict": (short, fz.ZSTD, past, len(raw) + 8),
           "truncated_entropy": (cut, fz.ZSTD, good, len(raw))}
    out = {k: (d, t, fz.frame_block(f, n), decompress(f, n, d))
           for k, (d, t, f, n) in out.items()}
    lz = bytes([0x0c]) + (4096 + 1).to_bytes(2, "little") + fl.emit(raw[16:], [])
    out["lz4_offset_past_dict"] = (rng.randbytes(4096), fl.LZ4, fl.frame(lz, len(raw)), None)
    return out
