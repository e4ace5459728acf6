"""LZ4 block streams from outside the project, and the decoder's spec.

`decode` is the acceptance rule of toplingdb_amd/csrc/dcw_lz4_dec.h in plain
Python; every C++ form must agree with it.  `emit` writes given matches
verbatim (directed streams; no matches: all literals), liblz4 is one more
encoder where it is installed, `malformed` hand-assembles the streams every
decoder must refuse.  A stored block of type
4 (LZ4) or 5 (LZ4HC) is `frame(stream, size)`: varint32(size) + stream.
"""
import ctypes

LZ4, LZ4HC = 4, 5


class Lz4Error(ValueError):
    pass


def put_varint32(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def frame(stream, size):
    return put_varint32(size) + stream


def unframe(payload):
    """-> (promised size, raw LZ4 block); at most 5 preamble bytes."""
    v = 0
    for i, b in enumerate(payload[:5]):
        v |= (b & 0x7f) << (7 * i)
        if not b & 0x80:
            return v & 0xffffffff, payload[i + 1:]
    raise Lz4Error("varint preamble")


def decode(s, size):
    """The spec: loop while input remains; token, literal length, literals;
    input exhausted -> the block ends; else offset, match length, match.
    Accepted iff the input is consumed exactly and `size` bytes came out."""
    out = bytearray()
    ip, n = 0, len(s)

    def ext(v, room):
        nonlocal ip
        while True:
            if ip >= n:
                raise Lz4Error("unterminated extension")
            b = s[ip]
            ip += 1
            v += b
            if v > room:
                raise Lz4Error("length beyond what is left")
            if b != 255:
                return v

    while ip < n:
        tok = s[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            ll = ext(ll, n - ip)
        if ll > n - ip or ll > size - len(out):
            raise Lz4Error("literals past the end")
        out += s[ip:ip + ll]
        ip += ll
        if ip == n:
            break
        if ip + 2 > n:
            raise Lz4Error("truncated offset")
        off = s[ip] | (s[ip + 1] << 8)
        ip += 2
        ml = (tok & 15) + 4
        if ml == 19:
            ml = ext(ml, size - len(out))
        if off == 0 or off > len(out) or ml > size - len(out):
            raise Lz4Error("bad match")
        for _ in range(ml):
            out.append(out[-off])
    if len(out) != size:
        raise Lz4Error("short of the promised size")
    return bytes(out)


def _length(out, v):
    """extension bytes of a nibble that said 15 (v = length - 15)"""
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)


def emit(raw, matches, final_token=False):
    """Directed-stream builder: `matches` = [(position, offset, length)] in
    position order, each written as one sequence exactly as given, the bytes
    between them as its literals.  A stream whose last match ends at
    len(raw) ends with zero final literals: no token follows, unless
    `final_token` asks for the empty last sequence (token 0)."""
    out = bytearray()
    at = 0
    for pos, off, ml in matches:
        assert at <= pos and 1 <= off <= pos and ml >= 4
        assert all(raw[pos + i] == raw[pos + i - off] for i in range(ml))
        ll = pos - at
        out.append((min(ll, 15) << 4) | min(ml - 4, 15))
        if ll >= 15:
            _length(out, ll - 15)
        out += raw[at:pos]
        out += bytes((off & 255, off >> 8))
        if ml - 4 >= 15:
            _length(out, ml - 19)
        at = pos + ml
    ll = len(raw) - at
    if ll or final_token or not matches:
        out.append(min(ll, 15) << 4)
        if ll >= 15:
            _length(out, ll - 15)
        out += raw[at:]
    return bytes(out)


def liblz4_encode(raw):
    """LZ4_compress_default, if liblz4 is installed; else None."""
    try:
        lib = ctypes.CDLL("liblz4.so.1")
    except OSError:
        return None
    cap = len(raw) + len(raw) // 255 + 16
    dst = ctypes.create_string_buffer(cap)
    got = lib.LZ4_compress_default(raw, dst, len(raw), cap)
    assert got > 0
    return dst.raw[:got]


POLICIES = {"all_literal": lambda raw: emit(raw, []), "liblz4": liblz4_encode}


def best(raw):
    """liblz4's stream where there is one, else all literals"""
    return liblz4_encode(raw) or emit(raw, [])


def malformed(raw):
    """name -> stored payload (preamble included) for one raw block of 200
    bytes or more.  Each is a bounds decision taken before any move."""
    size = len(raw)
    head = bytes([0xf0, 85]) + raw[:100]  # 100 literals; a match of 4 follows
    rest = emit(raw[104:], [])
    return {
        "offset_0": frame(head + bytes([0, 0]) + rest, size),
        "offset_gt_produced": frame(head + bytes([101, 0]) + rest, size),
        "literal_past_input": frame(bytes([0xf0, 200]) + raw[:150], size),
        "truncated_offset": frame(head + bytes([50]), size),
        "unterminated_literal_ext": frame(bytes([0xf0, 255, 255]), size),
        "unterminated_match_ext":
            frame(bytes([0xff, 85]) + raw[:100] + bytes([50, 0, 255, 255]),
                  size),
        "output_past_size": frame(emit(raw, []), size - 1),
        "match_past_size":  # 100 literals + a match of 12 into 110 bytes
            frame(bytes([0xf8, 85]) + raw[:100] + bytes([50, 0]), 110),
        "output_short_of_size": frame(emit(raw[:-1], []), size),
        "overlong_varint": b"\x80\x80\x80\x80\x80\x01" + emit(raw, []),
    }


MALFORMED_NAMES = tuple(malformed(bytes(200)))


# ---------------------------------------------------------------- the corpus
# Shared by test_lz4_input_cpu.py (every stored LZ4 block through the host
# decoders) and test_lz4_input_gpu.py (the same files through the worker).
import functools  # noqa: E402
import random  # noqa: E402

import foreign_corpus as fc  # noqa: E402
import oracle  # noqa: E402

DEC_MAX = fc.DEC_MAX


def build_pair(kvs, choose, **opts):
    """kvs as foreign_corpus.build_run takes them; choose(block index, raw)
    -> None (store raw) or (type, stream).  -> (kvs, sst, raw twin of the same
    entries, [(payload, raw)] of the compressed blocks)."""
    stored = []
    count = [0]

    def codec(raw):
        r = choose(count[0], raw)
        count[0] += 1
        if r is None:
            return None
        stored.append((frame(r[1], len(raw)), raw))
        return r[0], stored[-1][0]

    entries = [(oracle.make_ikey(k, s, t), v) for k, s, t, v in kvs]
    to = oracle.default_table_opts(**opts)
    return (kvs, oracle.build_sst(entries, to, data_block_codec=codec),
            oracle.build_sst(entries, to), stored)


def with_lz4_index(sst):
    """The same file with its index block stored as type 4, as real LZ4
    files have it: the coded block goes in front of a new footer that points
    at it (the old index block stays behind as dead bytes)."""
    foot = sst[-53:]
    vals, at = [], 1
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
    body = frame(best(index), len(index))
    csum = oracle.block_checksum(foot[0], body, LZ4)
    handles = b"".join(map(put_varint32, vals[:2] + [len(sst) - 53, len(body)]))
    return (sst[:-53] + body + bytes([LZ4]) + csum.to_bytes(4, "little") +
            foot[:1] + handles.ljust(40, b"\0") + foot[41:])


@functools.lru_cache(maxsize=None)
def policy_job(policy, btype=LZ4):
    """Type-5 files also carry an LZ4-coded index block."""
    rng = random.Random(0x4C + sorted(POLICIES).index(policy))
    job = [build_pair(kvs, lambda i, raw: (btype, POLICIES[policy](raw)),
                      block_size=4096)
           for kvs in fc.two_runs(900, 700, rng)]
    if btype == LZ4HC:
        job = [(k, with_lz4_index(s), t, st) for k, s, t, st in job]
    return job


# (literal length, offset, match length): the nibble and extension
# boundaries, the single-fetch boundary at 5/6, pattern doubling (offsets
# below 8) and the 8/16-byte switch
DIRECTED = ([(ll, 20, 8) for ll in (0, 5, 6, 14, 15, 16, 269, 270, 525)] +
            [(3, 20, ml) for ml in (4, 18, 19, 20, 273, 274)] +
            [(2, off, ml) for off in range(1, 18) for ml in (4, 8, 9, 17, 64)])
RESTART_TAIL = bytes(4) + b"\x01\x00\x00\x00"  # end of a one-restart block


def directed_value(ll, off, ml, rng):
    """-> (value, its two matches): random bytes, an anchor match of 4, `ll`
    literals, then the match (off, ml).  Positions are value-relative."""
    pre = rng.randbytes(max(off, 8))
    buf = bytearray(pre + pre[-4:] + rng.randbytes(ll))
    pos = len(buf)
    for _ in range(ml):
        buf.append(buf[-off])
    return bytes(buf), [(len(pre), 4, 4), (pos, off, ml)]


def directed_stream(raw, planned):
    """The block's stream with exactly the planned sequences of the values
    it holds, and, where the block's last 8 bytes occur earlier, a last
    match that ends the block with zero final literals."""
    matches = []
    for value, rel in planned:
        at = raw.find(value)
        if at >= 0:
            matches += [(at + p, off, ml) for p, off, ml in rel]
    matches.sort()
    n = len(raw)
    c = raw.rfind(raw[-8:], max(0, n - 8 - 65535), n - 1)
    if c >= 0 and (not matches or sum(matches[-1][::2]) <= n - 8):
        matches.append((n - 8, n - 8 - c, 8))
        directed_stream.ended_on_match += 1
    return emit(raw, matches)


directed_stream.ended_on_match = 0


@functools.lru_cache(maxsize=None)
def directed_job():
    rng = random.Random(0xD4)
    planned = [directed_value(*case, rng) for case in DIRECTED]
    kvs = [[], []]
    for i, (value, _) in enumerate(planned):
        kvs[i % 2].append((fc.ukey(i), 1 + i, fc.TYPE_VALUE,
                           value + (RESTART_TAIL if i % 3 == 0 else b"")))
    for i in range(0, len(planned), 20):  # run 1 shadows a few run-0 keys
        kvs[1].append((fc.ukey(i), 10000 + i, fc.TYPE_VALUE, b"new-%d" % i))
    for r, fill in enumerate(fc.two_runs(300, 200, rng)):  # ordinary entries
        kvs[r] += [(fc.ukey(1000 + int(k[1:])), s, t, v[:60])
                   for k, s, t, v in fill]
    return [build_pair(sorted(k), lambda i, raw: (
        LZ4, directed_stream(raw, planned)), block_size=4096,
        block_restart_interval=64) for k in kvs]


@functools.lru_cache(maxsize=None)
def decmax_job():
    """One entry per block (block_size 64).  Decoded sizes DEC_MAX - 1,
    DEC_MAX, DEC_MAX + 1 of compressible blocks, and all-literal blocks whose
    stream (token + 20 extension bytes + literals = size + 21) is DEC_MAX -
    1, DEC_MAX, DEC_MAX + 1 long while the decoded size stays below."""
    rng = random.Random(0xB4)
    pat = rng.randbytes(37)
    plan = [(True, us, (pat * 200)[:us - fc.ENTRY_OVERHEAD])
            for us in (DEC_MAX - 1, DEC_MAX, DEC_MAX + 1)]
    plan += [(False, us, rng.randbytes(us - fc.ENTRY_OVERHEAD))
             for us in (DEC_MAX - 22, DEC_MAX - 21, DEC_MAX - 20)]

    def choose(i, raw):  # one match over the periodic value, or all literals
        at = raw.find(pat) + 37
        return LZ4, emit(raw, [(at, 37, len(plan[i][2]) - 37)] * plan[i][0])

    kv0 = [(fc.ukey(10 * i), 1 + i, fc.TYPE_VALUE, v)
           for i, (_, _, v) in enumerate(plan)]
    v1 = fc.mixed_values(300, rng)
    kv1 = sorted([(fc.ukey(10 * i + 5), 5000 + i, fc.TYPE_VALUE, v1[i])
                  for i in range(300)] +
                 [(fc.ukey(10), 9000, fc.TYPE_DELETION, b"")])
    run0 = build_pair(kv0, choose, block_size=64)
    sizes = [(len(unframe(p)[1]), len(raw)) for p, raw in run0[3]]
    assert [u for _, u in sizes] == [us for _, us, _ in plan]
    assert [n for n, _ in sizes[3:]] == [DEC_MAX - 1, DEC_MAX, DEC_MAX + 1]
    assert all(n < 1000 for n, _ in sizes[:3])
    return [run0,
            build_pair(kv1, lambda i, raw: (LZ4, best(raw)), block_size=4096)]


@functools.lru_cache(maxsize=None)
def big_job():
    """A 128 KiB input block: one value repeats 400 of its bytes 65535 bytes
    later (the largest offset, a match extension over 255), the rest of the
    block is literals (extensions of hundreds of bytes, global path)."""
    rng = random.Random(0xB16)
    rep = rng.randbytes(400)
    big = rep + rng.randbytes(65535 - 400) + rep
    kv0, kv1 = fc.two_runs(600, 400, rng)
    kv0 = sorted(kv0 + [(fc.ukey(1), 50000, fc.TYPE_VALUE, big)])

    def choose(i, raw):
        at = raw.find(big)
        return LZ4, emit(raw, [(at + 65535, 65535, 400)] if at >= 0 else [])

    return [build_pair(kv0, choose, block_size=131072),
            build_pair(kv1, lambda i, raw: (LZ4HC, best(raw)),
                       block_size=4096)]


@functools.lru_cache(maxsize=None)
def alternating_job():
    """Run 0: raw and LZ4 blocks alternate inside the file; run 1: snappy
    (its own twin)."""
    rng = random.Random(0xA4)
    kv0, kv1 = fc.two_runs(900, 700, rng)
    entries = [(oracle.make_ikey(k, s, t), v) for k, s, t, v in kv1]
    snap = oracle.build_sst(entries, oracle.default_table_opts(compression=1))
    return [build_pair(kv0, lambda i, raw: (LZ4, best(raw)) if i % 2 else None,
                       block_size=4096),
            (kv1, snap, snap, [])]


@functools.lru_cache(maxsize=None)
def malformed_input(name):
    """-> a small file whose second data block is the named malformed
    payload behind a valid checksum."""
    rng = random.Random(0xE4)
    kvs = [(fc.ukey(i), 1 + i, fc.TYPE_VALUE, v)
           for i, v in enumerate(fc.mixed_values(150, rng))]
    entries = [(oracle.make_ikey(k, s, t), v) for k, s, t, v in kvs]
    count = [0]

    def codec(raw):
        count[0] += 1
        if count[0] == 2:
            return LZ4, malformed(raw)[name]
        return LZ4, frame(best(raw), len(raw))

    sst = oracle.build_sst(entries, oracle.default_table_opts(block_size=4096),
                           data_block_codec=codec)
    assert count[0] >= 3
    return sst


def streams():
    """-> ([(payload, raw)] every decoder must decode, [payload] every
    decoder must refuse): all stored blocks of the jobs above, the edge
    forms, the malformed set at an LDS and at a global-path size."""
    jobs = [policy_job(p) for p in sorted(POLICIES)
            if POLICIES[p](b"probe") is not None]
    jobs += [directed_job(), decmax_job(), big_job(), alternating_job()]
    good = [s for job in jobs for run in job for s in run[3]]
    rng = random.Random(0x57)
    raw = rng.randbytes(40) * 3
    good += [(frame(b"", 0), b""), (frame(b"\x00", 0), b""),
             (frame(emit(raw, [(40, 40, 80)]), 120), raw),
             (frame(emit(raw, [(40, 40, 80)], final_token=True), 120), raw)]
    bad = [p for n in (1000, 6000)
           for p in malformed(rng.randbytes(n)).values()]
    return good, bad
