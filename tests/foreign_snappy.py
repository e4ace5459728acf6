"""Plain-Python snappy helpers for the foreign-input tests (no GPU, no
native code).  A from-scratch restatement of the public snappy block format:

  stream  = varint32(uncompressed length) op*
  literal = tag (len-1)<<2 | 0, with len-1 < 60 inline, else tag (59+k)<<2
            followed by k = 1..4 little-endian bytes of len-1, then the bytes
  copy 1  = tag (offset>>8)<<5 | (len-4)<<2 | 1, one offset byte
            (4 <= len <= 11, offset < 2048)
  copy 2  = tag (len-1)<<2 | 2, two little-endian offset bytes (len <= 64)
  copy 3  = tag (len-1)<<2 | 3, four little-endian offset bytes (len <= 64)

decode() is the independent reference: the oracle decoder and the GPU
decoders are both checked against it.  The encoder policies exist because the
project's own codec emits a narrow subset of the format (64 independent
segments, so no long literals, no chunked matches, no 4-byte offsets); these
emit what a whole-block encoder emits, and then some.
"""
import random
from collections import Counter, namedtuple


class SnappyError(ValueError):
    pass


def put_varint32(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def read_preamble(stream):
    """-> (uncompressed length, position of the first op)."""
    ulen = 0
    for i in range(5):
        if i >= len(stream):
            raise SnappyError("preamble truncated")
        b = stream[i]
        ulen |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            if ulen >> 32:
                raise SnappyError("preamble overflows 32 bits")
            return ulen, i + 1
    raise SnappyError("preamble longer than 5 bytes")


# kind: "lit" or "copy"; form: literal = number of length-extension bytes
# (0..4), copy = tag (1..3); pos/end: the op's first byte / one past its last
Op = namedtuple("Op", "kind length offset form pos end")


def parse(stream):
    """-> (ulen, [Op]).  Validates exactly what decode() validates."""
    ulen, ip = read_preamble(stream)
    n = len(stream)
    produced = 0
    ops = []
    while ip < n:
        pos = ip
        tag = stream[ip]
        ip += 1
        if tag & 3 == 0:
            length = (tag >> 2) + 1
            ext = 0
            if length > 60:
                ext = length - 60
                if ip + ext > n:
                    raise SnappyError("literal length bytes past the input")
                length = int.from_bytes(stream[ip:ip + ext], "little") + 1
                ip += ext
            if ip + length > n:
                raise SnappyError("literal runs past the input")
            if produced + length > ulen:
                raise SnappyError("literal runs past the announced length")
            ip += length
            ops.append(Op("lit", length, 0, ext, pos, ip))
        else:
            form = tag & 3
            if form == 1:
                length = ((tag >> 2) & 7) + 4
                if ip + 1 > n:
                    raise SnappyError("copy-1 header past the input")
                offset = ((tag >> 5) << 8) | stream[ip]
                ip += 1
            else:
                length = (tag >> 2) + 1
                nb = 2 if form == 2 else 4
                if ip + nb > n:
                    raise SnappyError("copy-%d header past the input" % form)
                offset = int.from_bytes(stream[ip:ip + nb], "little")
                ip += nb
            if offset == 0:
                raise SnappyError("copy offset 0")
            if offset > produced:
                raise SnappyError("copy offset before the output start")
            if produced + length > ulen:
                raise SnappyError("copy runs past the announced length")
            ops.append(Op("copy", length, offset, form, pos, ip))
        produced += length
    if produced != ulen:
        raise SnappyError("stream produced %d bytes, announced %d" %
                          (produced, ulen))
    return ulen, ops


def decode(stream):
    """Byte-at-a-time reference decoder; raises SnappyError on every
    malformed stream."""
    ulen, ip = read_preamble(stream)
    n = len(stream)
    out = bytearray()
    while ip < n:
        tag = stream[ip]
        ip += 1
        if tag & 3 == 0:
            length = (tag >> 2) + 1
            if length > 60:
                ext = length - 60
                if ip + ext > n:
                    raise SnappyError("literal length bytes past the input")
                length = 0
                for i in range(ext):
                    length |= stream[ip + i] << (8 * i)
                length += 1
                ip += ext
            if ip + length > n:
                raise SnappyError("literal runs past the input")
            if len(out) + length > ulen:
                raise SnappyError("literal runs past the announced length")
            for i in range(length):
                out.append(stream[ip + i])
            ip += length
        else:
            form = tag & 3
            if form == 1:
                length = ((tag >> 2) & 7) + 4
                if ip >= n:
                    raise SnappyError("copy-1 header past the input")
                offset = ((tag >> 5) << 8) | stream[ip]
                ip += 1
            elif form == 2:
                length = (tag >> 2) + 1
                if ip + 2 > n:
                    raise SnappyError("copy-2 header past the input")
                offset = stream[ip] | (stream[ip + 1] << 8)
                ip += 2
            else:
                length = (tag >> 2) + 1
                if ip + 4 > n:
                    raise SnappyError("copy-3 header past the input")
                offset = (stream[ip] | (stream[ip + 1] << 8) |
                          (stream[ip + 2] << 16) | (stream[ip + 3] << 24))
                ip += 4
            if offset == 0:
                raise SnappyError("copy offset 0")
            if offset > len(out):
                raise SnappyError("copy offset before the output start")
            if len(out) + length > ulen:
                raise SnappyError("copy runs past the announced length")
            for _ in range(length):
                out.append(out[-offset])
    if len(out) != ulen:
        raise SnappyError("stream produced %d bytes, announced %d" %
                          (len(out), ulen))
    return bytes(out)


def walk(stream):
    """Classify every op of a valid stream.  Counter keys: ops, lit_ext0
    (short header) .. lit_ext4, copy_tag1..copy_tag3, off_1_7, off_8_15,
    off_ge16, overlap (offset < len)."""
    c = Counter()
    for op in parse(stream)[1]:
        c["ops"] += 1
        if op.kind == "lit":
            c["lit_ext%d" % op.form] += 1
        else:
            c["copy_tag%d" % op.form] += 1
            if op.offset < 8:
                c["off_1_7"] += 1
            elif op.offset < 16:
                c["off_8_15"] += 1
            else:
                c["off_ge16"] += 1
            if op.offset < op.length:
                c["overlap"] += 1
    return c


def chunked_matches(ops):
    """Lengths (in ops) of the runs of consecutive copies that continue one
    match: same offset, every piece but the last 64 or 60 bytes long."""
    runs = []
    cur = 0
    prev = None
    for op in ops:
        if (op.kind == "copy" and prev is not None and prev.kind == "copy" and
                prev.offset == op.offset and prev.length in (60, 64)):
            cur += 1
        else:
            if cur > 1:
                runs.append(cur)
            cur = 1 if op.kind == "copy" else 0
        prev = op
    if cur > 1:
        runs.append(cur)
    return runs


# ---------------------------------------------------------------- encoders
def _emit_literal(out, data, lo, hi):
    n = hi - lo
    if n <= 0:
        return
    m = n - 1
    if m < 60:
        out.append(m << 2)
    else:
        ext = m.to_bytes((m.bit_length() + 7) // 8, "little")
        out.append((59 + len(ext)) << 2)
        out += ext
    out += data[lo:hi]


def _emit_copy_piece(out, offset, length, tag3):
    if tag3 or offset >= 65536:
        out.append(((length - 1) << 2) | 3)
        out += offset.to_bytes(4, "little")
    elif 4 <= length <= 11 and offset < 2048:
        out.append(((offset >> 8) << 5) | ((length - 4) << 2) | 1)
        out.append(offset & 0xFF)
    else:
        out.append(((length - 1) << 2) | 2)
        out += offset.to_bytes(2, "little")


def _emit_copy(out, offset, length, tag3=lambda: False):
    """Real-snappy chunking: 64s while >= 68 remain, then 60 if more than 64
    remain, then the rest (so no piece is shorter than 4)."""
    while length >= 68:
        _emit_copy_piece(out, offset, 64, tag3())
        length -= 64
    if length > 64:
        _emit_copy_piece(out, offset, 60, tag3())
        length -= 60
    _emit_copy_piece(out, offset, length, tag3())


def _match_len(data, cand, p, n, limit):
    length = 4
    while length < limit and p + length < n and \
            data[cand + length] == data[p + length]:
        length += 1
    return length


def greedy(data, seed=0, tag3_fraction=0.0):
    """Whole-block greedy matcher over a last-occurrence table of 4-byte
    grams (every position is entered, matched or not)."""
    rng = random.Random(seed)
    tag3 = (lambda: rng.random() < tag3_fraction) if tag3_fraction else \
        (lambda: False)
    n = len(data)
    out = bytearray(put_varint32(n))
    table = {}
    p = lit = 0
    while p + 4 <= n:
        gram = data[p:p + 4]
        cand = table.get(gram)
        table[gram] = p
        if cand is None:
            p += 1
            continue
        length = _match_len(data, cand, p, n, n)
        _emit_literal(out, data, lit, p)
        _emit_copy(out, p - cand, length, tag3)
        for q in range(p + 1, min(p + length, n - 3)):
            table[data[q:q + 4]] = q
        p += length
        lit = p
    _emit_literal(out, data, lit, n)
    return bytes(out)


def greedy_tag3(data, seed=0):
    """greedy, with a seeded tenth of the copies in the 5-byte form (small
    offsets in that form are legal snappy)."""
    return greedy(data, seed, tag3_fraction=0.1)


def all_literal(data, seed=0):
    """One literal covering the whole block."""
    out = bytearray(put_varint32(len(data)))
    _emit_literal(out, data, 0, len(data))
    return bytes(out)


def fragmented(data, seed=0):
    """Literals of 1-3 bytes alternating with short copies where a match is
    available: many ops per block, and on poorly compressible data a stream
    longer than the raw block."""
    rng = random.Random(seed)
    n = len(data)
    out = bytearray(put_varint32(n))
    table = {}

    def enter(lo, hi):
        for q in range(lo, min(hi, n - 3)):
            table[data[q:q + 4]] = q

    p = 0
    while p < n:
        k = min(rng.randint(1, 3), n - p)
        _emit_literal(out, data, p, p + k)
        enter(p, p + k)
        p += k
        if p + 4 <= n:
            cand = table.get(data[p:p + 4])
            if cand is not None:
                length = _match_len(data, cand, p, n, rng.randint(4, 8))
                _emit_copy(out, p - cand, length)
                enter(p, p + length)
                p += length
    return bytes(out)


POLICIES = {
    "greedy": greedy,
    "greedy_tag3": greedy_tag3,
    "all_literal": all_literal,
    "fragmented": fragmented,
}


# ------------------------------------------------------- directed data
DIRECTED_OFFSETS = tuple(range(1, 18)) + (2047, 2048)
DIRECTED_LENGTHS = (4, 7, 8, 9, 11, 12, 15, 16, 17, 60, 63, 64, 65, 67, 68,
                    129)


def directed_value(offset, length, rng):
    """`offset` bytes, their periodic extension to offset+length bytes, then
    a byte that breaks the period: the greedy policy emits a copy with
    exactly that offset and length.  Short patterns use distinct bytes so
    the true period is `offset`; no pattern byte is 0, the byte that ends
    the internal key in front of a value, so the match cannot start early."""
    if offset <= 255:
        pat = bytes(rng.sample(range(1, 256), offset))
    else:
        pat = bytes(rng.randrange(1, 256) for _ in range(offset))
    total = offset + length
    body = (pat * (total // offset + 1))[:total]
    breaker = pat[total % offset] ^ 0x55
    return body + bytes([breaker])
