"""Raw deflate streams by Python's zlib module, the foreign encoder and the
referee of the type-2 (kZlibCompression) input decoders: named cases, and the
jobs built from them.  A stored block is foreign_lz4.frame(stream, size):
varint32(size) + one raw deflate stream."""
import functools
import random
import zlib

import foreign_corpus as fc
import foreign_lz4 as fl
import oracle

ZLIB = 2
DEC_MAX = fc.DEC_MAX


def deflate(raw, level=6, wbits=-14, strategy=zlib.Z_DEFAULT_STRATEGY, cuts=()):
    """a Z_FULL_FLUSH at each of `cuts`: the block ends, an empty stored follows"""
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    out, at = b"", 0
    for cut in cuts:
        out += c.compress(raw[at:cut]) + c.flush(zlib.Z_FULL_FLUSH)
        at = cut
    return out + c.compress(raw[at:]) + c.flush()


def verdict(stream, size):
    """zlib's: the bytes iff the stream reaches its end with exactly `size`."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(stream))
    except zlib.error:
        return None
    return out if d.eof and len(out) == size else None


POLICIES = {
    "stored": lambda raw: deflate(raw, 0),
    "fixed": lambda raw: deflate(raw, strategy=zlib.Z_FIXED),
    "dynamic_6": deflate,
    "dynamic_9_w15": lambda raw: deflate(raw, 9, -15),
    "huffman_only": lambda raw: deflate(raw, strategy=zlib.Z_HUFFMAN_ONLY),
    "rle": lambda raw: deflate(raw, strategy=zlib.Z_RLE),
    # a short head and a short tail (zlib codes them fixed), the body dynamic,
    # an empty stored block behind each cut
    "three_kinds": lambda raw: deflate(raw, cuts=(12, len(raw) - 9)),
}


def fibonacci_bytes(terms=16):
    """4179 bytes of frequencies 1, 2, 3, 5, ... (end-of-block is the series'
    first 1; two bytes of frequency 1 tie and zlib's tree stays shallow): a
    free Huffman code is deeper than 15, so zlib hands out 15-bit codes."""
    a, b, out = 1, 2, bytearray()
    for i in range(terms):
        out += bytes([65 + i]) * a
        a, b = b, a + b
    random.Random(0xF1B).shuffle(out)
    return bytes(out)


def copies_of_copies(rng):
    """each match of a batch reads what the match before it wrote"""
    out = bytearray(rng.randbytes(40))
    for i in range(30):
        out += out[-40:-4] + bytes([i])
    return bytes(out)


def word_text(n, rng, vocabulary=700):
    words = [rng.randbytes(rng.randrange(3, 12)) for _ in range(vocabulary)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + b" "
    return bytes(out[:n])


def huff(code, nbits):
    """a Huffman code, first bit first, as (value, nbits) of the bit writer"""
    return int(format(code, "0%db" % nbits)[::-1], 2), nbits


def pack(fields):
    """(value, nbits) fields, lowest bit first: malformed streams only"""
    v = at = 0
    for val, nbits in fields:
        v |= val << at
        at += nbits
    return v.to_bytes((at + 7) // 8, "little")


def _dynamic_header(hclen, cl_lens):
    """final dynamic block, HLIT 257, HDIST 1, the code-length-code lengths"""
    return [(1, 1), (2, 2), (0, 5), (0, 5), (hclen - 4, 4)] + [(v, 3) for v in cl_lens]


def malformed(raw):
    """name -> (stream, promised size) that every decoder refuses; `raw`: 300
    bytes or more of compressible text."""
    good, stored = deflate(raw), deflate(raw, 0)
    cl01 = [0, 0, 0, 1] + [0] * 13 + [1]  # symbols 0 and 1, one bit each
    return {
        # fixed block: literal 'a', length 3 at distance 2, end of block
        "distance_beyond_start": (pack([(1, 1), (1, 2), huff(0x30 + 97, 8), huff(1, 7),
                                        huff(1, 5), huff(0, 7)]), 4),
        "btype_3": (b"\x07" + good[1:], len(raw)),
        "len_nlen_mismatch": (stored[:3] + bytes([stored[3] ^ 0x10]) + stored[4:], len(raw)),
        # 257 literal/length symbols of length 1
        "oversubscribed_lengths": (pack(_dynamic_header(18, cl01) + [(1, 1)] * 258 + [(0, 8)]),
                                   1),
        # code-length code of the symbols 0 and 16; the first symbol is a 16
        "repeat_at_0": (pack(_dynamic_header(4, [1, 0, 0, 1]) + [(1, 1), (0, 2)] + [(0, 16)]), 1),
        "cut_short": (good[:len(good) // 2], len(raw)),
        "size_too_small": (good, len(raw) - 1),
        "size_too_large": (good, len(raw) + 1),
    }


MALFORMED_NAMES = tuple(malformed(bytes(range(60)) * 5))
TRAILING = b"\xaa\xbb\xcc"  # behind the final block: accepted


def flips(count=240):
    """seeded single-bit flips of one level-6 stream of 4 KiB of word text"""
    rng = random.Random(0xF11)
    raw = word_text(4096, rng)
    s = deflate(raw)
    out = []
    for _ in range(count):
        t = bytearray(s)
        t[rng.randrange(len(s))] ^= 1 << rng.randrange(8)
        out.append((bytes(t), len(raw), verdict(t, len(raw))))
    return out


# ------------------------------------------------------------------ the jobs
def codec(encode=deflate):
    return lambda i, raw: (ZLIB, encode(raw))


@functools.lru_cache(maxsize=None)
def policy_job(policy):
    rng = random.Random(0x2B + sorted(POLICIES).index(policy))
    return [fl.build_pair(kvs, codec(POLICIES[policy]), block_size=4096)
            for kvs in fc.two_runs(300, 200, rng)]


@functools.lru_cache(maxsize=None)
def fibonacci_job():
    """run 0: the Fibonacci value in a block of its own, literals only"""
    rng = random.Random(0xF1)
    kv0, kv1 = fc.two_runs(200, 150, rng)
    kv0 = sorted(kv0 + [(fc.ukey(1), 70000, fc.TYPE_VALUE, fibonacci_bytes())])
    return [fl.build_pair(kv0, codec(POLICIES["huffman_only"]), block_size=4096),
            fl.build_pair(kv1, codec(), block_size=4096)]


@functools.lru_cache(maxsize=None)
def edge_job():
    """One entry per block: decoded DEC_MAX and DEC_MAX + 1; a stream within
    DEC_MAX that decodes to more; a stored block the other way round."""
    rng = random.Random(0xED)
    plan = [(us, word_text(us - fc.ENTRY_OVERHEAD, rng, 100), lvl)
            for us, lvl in ((DEC_MAX, 6), (DEC_MAX + 1, 6), (9000, 6), (DEC_MAX - 2, 0))]
    kv0 = [(fc.ukey(10 * i), 1 + i, fc.TYPE_VALUE, v) for i, (_, v, _) in enumerate(plan)]
    run0 = fl.build_pair(kv0, lambda i, raw: (ZLIB, deflate(raw, plan[i][2])), block_size=64)
    sizes = [(len(fl.unframe(p)[1]), len(raw)) for p, raw in run0[3]]
    assert [u for _, u in sizes] == [us for us, _, _ in plan]
    assert sizes[2][0] <= DEC_MAX < sizes[3][0]
    kv1 = [(fc.ukey(10 * i + 5), 5000 + i, fc.TYPE_VALUE, v)
           for i, v in enumerate(fc.mixed_values(150, rng))]
    return [run0, fl.build_pair(kv1, codec(), block_size=4096)]


@functools.lru_cache(maxsize=None)
def large_job(name):
    """64 KiB blocks, or one value of 200000 bytes of word text: several
    deflate blocks with matches up to 32768 back across them"""
    rng = random.Random(0x1A + len(name))
    kv0, kv1 = fc.two_runs(400, 300, rng, far=(30, 350))
    size = 65536
    if name == "value_200k":
        kv0 = sorted(kv0 + [(fc.ukey(1), 60000, fc.TYPE_VALUE, word_text(200000, rng))])
        size = 4096
    return [fl.build_pair(kv0, codec(lambda raw: deflate(raw, 6, -15)), block_size=size),
            fl.build_pair(kv1, codec(), block_size=4096)]


def with_zlib_index(sst):
    """the file with its index block stored again as type 2, and a new footer"""
    foot, vals, at = sst[-53:], [], 1
    for _ in range(4):  # metaindex offset, size; index offset, size
        v = shift = 0
        while True:
            b = foot[at]
            at += 1
            v |= (b & 0x7f) << shift
            shift += 7
            if not b & 0x80:
                break
        vals.append(v)
    index = sst[vals[2]:vals[2] + vals[3]]
    body = fl.frame(deflate(index), len(index))
    csum = oracle.block_checksum(foot[0], body, ZLIB)
    handles = b"".join(map(fl.put_varint32, vals[:2] + [len(sst) - 53, len(body)]))
    return (sst[:-53] + body + bytes([ZLIB]) + csum.to_bytes(4, "little") +
            foot[:1] + handles.ljust(40, b"\0") + foot[41:])


@functools.lru_cache(maxsize=None)
def mixed_job():
    """run 0: raw, zlib, LZ4 blocks in turn, zlib-coded index; run 1: snappy"""
    rng = random.Random(0xA2)
    kv0, kv1 = fc.two_runs(450, 350, rng)
    entries = [(oracle.make_ikey(k, s, t), v) for k, s, t, v in kv1]
    snap = oracle.build_sst(entries, oracle.default_table_opts(compression=1))
    k, sst, twin, stored = fl.build_pair(
        kv0, lambda i, raw: (None, (ZLIB, deflate(raw)), (fl.LZ4, fl.best(raw)))[i % 3],
        block_size=4096)
    return [(k, with_zlib_index(sst), twin, stored), (kv1, snap, snap, [])]


@functools.lru_cache(maxsize=None)
def one_block_input(stream, size):
    """-> a small file whose second data block is the given stream"""
    rng = random.Random(0xE2)
    entries = [(oracle.make_ikey(fc.ukey(i), 1 + i, fc.TYPE_VALUE), v)
               for i, v in enumerate(fc.mixed_values(150, rng))]
    count = [0]

    def block(raw):
        count[0] += 1
        if count[0] == 2:
            return ZLIB, fl.frame(stream, size or len(raw))
        return ZLIB, fl.frame(deflate(raw), len(raw))

    sst = oracle.build_sst(entries, oracle.default_table_opts(block_size=4096),
                           data_block_codec=block)
    assert count[0] >= 3
    return sst


def streams():
    """-> [(stream, size, bytes or None)]: all of the above"""
    jobs = [policy_job(p) for p in sorted(POLICIES)]
    jobs += [fibonacci_job(), edge_job(), large_job("block_64k"), large_job("value_200k"),
             mixed_job()]
    recs = []
    for job in jobs:
        for run in job:
            for payload, raw in run[3]:
                size, s = fl.unframe(payload)
                if verdict(s, size) == raw:  # mixed_job also stores LZ4 blocks
                    recs.append((s, size, raw))
    rng = random.Random(0x57)
    text = word_text(3000, rng)
    for raw in (b"", b"x", fibonacci_bytes(), copies_of_copies(rng), text):
        recs += [(enc(raw), len(raw), raw) for enc in POLICIES.values() if len(raw) > 30]
        recs.append((deflate(raw) + TRAILING, len(raw), raw))
    recs += [(s, size, None) for s, size in malformed(text).values()]
    return recs + flips()
