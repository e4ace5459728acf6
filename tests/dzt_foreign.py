"""Foreign DcwZipTable ("DZT1") inputs for the DZT-input tests: take a DZT
file apart, put it back together with every checksum valid, re-encode its
value blocks through a plain-Python dict-snappy encoder whose op forms the
caller selects, and classify the ops of a stream.  Format: oracle/dzt.c
header comment; codec: "DZT dict codec v1" (virtual stream dict || block).

The oracle's own encoder emits almost only 2-byte-offset dict copies, so
the decoder classes the worker must accept come from the encoder here."""
import random
import struct
from collections import Counter

import oracle

FOOTER = 96
MAGIC = 0x313050495A574344
VB_ULEN_MAX = 16384


# ------------------------------------------------------------ file <-> parts
class Dzt:
    """The sections of one DZT file, editable; build() reassembles them and
    recomputes the index, the footer offsets and every checksum."""

    def __init__(self, data: bytes):
        f = data[-FOOTER:]
        (dict_off, value_off, kindex_off, vindex_off, props_off,
         props_size) = struct.unpack_from("<6Q", f, 0)
        self.ct, self.version = struct.unpack_from("<II", f, 68)
        assert struct.unpack_from("<Q", f, 88)[0] == MAGIC
        self.key_area = bytearray(data[:dict_off])
        self.dict = data[dict_off:value_off]
        value_area = data[value_off:kindex_off]
        kindex = data[kindex_off:vindex_off]
        vindex = data[vindex_off:props_off]
        self.props = bytearray(data[props_off:props_off + props_size])
        self.n, nkb, nvb = struct.unpack_from("<3Q", self.props, 0)
        self.U = struct.unpack_from("<I", self.props, 72)[0]
        ks = self.U + 28
        self.kblocks = []  # [first_ikey, koff, ksize, first_rank]
        for i in range(nkb):
            e = kindex[i * ks:(i + 1) * ks]
            koff, ksize, fr = struct.unpack_from("<QIQ", e, self.U + 8)
            self.kblocks.append([e[:self.U + 8], koff, ksize, fr])
        self.vblocks = []  # [btype, body, ulen, first_rank]
        for i in range(nvb):
            voff, csize, ulen, fr = struct.unpack_from("<QIIQ", vindex, i * 24)
            self.vblocks.append([value_area[voff + csize],
                                 value_area[voff:voff + csize], ulen, fr])
        # knobs for malformed files: written as given, under valid checksums
        self.kindex_override = None
        self.vindex_patch = {}  # block -> dict(voff=, csize=, ulen=, first_rank=)

    def raw_block(self, i) -> bytes:
        btype, body, ulen, _ = self.vblocks[i]
        if btype == 0:
            return bytes(body)
        return oracle.snappy_uncompress_dict(self.dict, bytes(body))

    def build(self) -> bytes:
        cs = lambda b, last=0: oracle.block_checksum(self.ct, bytes(b), last)
        value_area = bytearray()
        vindex = bytearray()
        for i, (btype, body, ulen, fr) in enumerate(self.vblocks):
            row = dict(voff=len(value_area), csize=len(body), ulen=ulen,
                       first_rank=fr)
            row.update(self.vindex_patch.get(i, {}))
            vindex += struct.pack("<QIIQ", row["voff"], row["csize"],
                                  row["ulen"], row["first_rank"])
            value_area += bytes(body) + bytes([btype])
            value_area += struct.pack("<I", cs(body, btype))
        kindex = bytearray()
        for first_ikey, koff, ksize, fr in (self.kindex_override
                                            or self.kblocks):
            kindex += bytes(first_ikey) + struct.pack("<QIQ", koff, ksize, fr)
        struct.pack_into("<Q", self.props, 24, len(self.dict))
        dict_off = len(self.key_area)
        value_off = dict_off + len(self.dict)
        kindex_off = value_off + len(value_area)
        vindex_off = kindex_off + len(kindex)
        props_off = vindex_off + len(vindex)
        footer = struct.pack("<6Q", dict_off, value_off, kindex_off,
                             vindex_off, props_off, len(self.props))
        footer += struct.pack("<5I", cs(self.key_area), cs(self.dict),
                              cs(kindex), cs(vindex), cs(self.props))
        footer += struct.pack("<IIIQQ", self.ct, self.version, 0, 0, MAGIC)
        assert len(footer) == FOOTER
        return (bytes(self.key_area) + bytes(self.dict) + bytes(value_area)
                + bytes(kindex) + bytes(vindex) + bytes(self.props) + footer)


def rewrite(data: bytes, encoder, dictionary: bytes = None) -> bytes:
    """Re-encode every value block of a DZT file: encoder(dict, raw) ->
    (btype, body).  With `dictionary` the file's dict is replaced too."""
    z = Dzt(data)
    raws = [z.raw_block(i) for i in range(len(z.vblocks))]
    if dictionary is not None:
        assert len(dictionary) <= 49152
        z.dict = bytes(dictionary)
    for i, raw in enumerate(raws):
        btype, body = encoder(z.dict, raw)
        z.vblocks[i][0] = btype
        z.vblocks[i][1] = bytes(body)
    return z.build()


# ------------------------------------------------------------------ encoder
def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def emit_literal(out, lit: bytes, ext=None):
    """ext = number of length bytes (0..4); None = the shortest form."""
    if not lit:
        return
    n = len(lit) - 1
    if ext is None:
        ext = 0 if n < 60 else (n.bit_length() + 7) // 8
    if ext == 0:
        assert n < 60
        out.append(n << 2)
    else:
        assert n < (1 << (8 * ext))
        out.append((59 + ext) << 2)
        out += n.to_bytes(ext, "little")
    out += lit


def emit_copy(out, offset, length, form=None):
    """form 1/2/3 = 1-, 2-, 4-byte-offset copy; None = the smallest that
    fits.  Lengths over 64 go out in chunks (form 1 only fits 4..11)."""
    while length > 0:
        f = form
        chunk = min(length, 64)
        if f == 1 and not (4 <= chunk <= 11 and offset < 2048):
            f = None
        if f is None:
            if 4 <= chunk <= 11 and offset < 2048 and length == chunk:
                f = 1
            else:
                f = 2 if offset < 65536 else 3
        if f == 2 and offset >= 65536:
            f = 3
        if f == 1:
            out.append(1 | ((chunk - 4) << 2) | ((offset >> 8) << 5))
            out.append(offset & 0xFF)
        elif f == 2:
            out.append(2 | ((chunk - 1) << 2))
            out += offset.to_bytes(2, "little")
        else:
            out.append(3 | ((chunk - 1) << 2))
            out += offset.to_bytes(4, "little")
        length -= chunk


def encode(dictionary: bytes, raw: bytes, mode="greedy", seed=0) -> bytes:
    """Dict-snappy stream for `raw`.  Modes:
      all_literal  no copies; literal length forms 0..4 bytes in rotation
      greedy       nearest match in dict || block, shortest forms
      tag3         as greedy, every copy in the 4-byte-offset form
      tag2         as greedy, no 1-byte-offset copies
      short_lits   as greedy, literals cut to <= 7 bytes (many ops)"""
    out = bytearray(_varint(len(raw)))
    if mode == "all_literal":
        rng = random.Random(seed)
        p, k = 0, 0
        while p < len(raw):
            ext = k % 5
            k += 1
            ln = min(len(raw) - p, rng.randint(1, (60, 256, 700, 700, 700)[ext]))
            emit_literal(out, raw[p:p + ln], ext)
            p += ln
        return bytes(out)
    form = {"tag3": 3, "tag2": 2}.get(mode)
    D = len(dictionary)
    v = dictionary + raw
    tab = {}
    for p in range(0, D - 3):
        tab[v[p:p + 4]] = p
    p = lit = D
    end = len(v)

    def flush(upto):
        chunk = 7 if mode == "short_lits" else 1 << 30
        q = lit
        while q < upto:
            emit_literal(out, v[q:min(upto, q + chunk)])
            q += chunk

    while p + 4 <= end:
        w = v[p:p + 4]
        c = tab.get(w)
        tab[w] = p
        if c is None:
            p += 1
            continue
        ln = 4
        while p + ln < end and v[c + ln] == v[p + ln]:
            ln += 1
        flush(p)
        emit_copy(out, p - c, ln, form)
        # keep the table warm inside the match (periodic data stays nearest)
        for q in range(p + 1, min(p + ln, end - 3)):
            tab[v[q:q + 4]] = q
        p += ln
        lit = p
    flush(end)
    return bytes(out)


def encoder(mode, seed=0):
    """-> encoder(dict, raw) for rewrite(); empty blocks stay raw like the
    builder's, everything else is stored compressed whatever its size."""
    def enc(dictionary, raw):
        if not raw:
            return 0, b""
        return 2, encode(dictionary, raw, mode, seed + len(raw))
    return enc


MODES = ("all_literal", "greedy", "tag3", "tag2", "short_lits")


# --------------------------------------------------------------- classifier
class StreamError(ValueError):
    pass


def classify(stream: bytes, dict_size: int) -> Counter:
    """Op classes of one dict-snappy stream (and a full validity check of
    its structure).  Classes: lit_ext0..lit_ext4; copy_tag1/2/3; dict_only,
    dict_into_block, in_block; overlap_<k> for in-block copies with
    offset k < length, k in 1..16."""
    c = Counter()
    ulen = shift = ip = 0
    while True:
        if ip >= len(stream) or shift > 28:
            raise StreamError("preamble")
        b = stream[ip]
        ip += 1
        ulen |= (b & 0x7F) << shift
        if not b & 0x80:
            break
        shift += 7
    op = 0
    n = len(stream)
    while ip < n:
        tag = stream[ip]
        ip += 1
        if tag & 3 == 0:
            ln = (tag >> 2) + 1
            ext = 0
            if ln > 60:
                ext = ln - 60
                if ip + ext > n:
                    raise StreamError("truncated literal length")
                ln = int.from_bytes(stream[ip:ip + ext], "little") + 1
                ip += ext
            if ip + ln > n or op + ln > ulen:
                raise StreamError("literal overrun")
            c["lit_ext%d" % ext] += 1
            ip += ln
            op += ln
            continue
        form = tag & 3
        if form == 1:
            ln = ((tag >> 2) & 7) + 4
            need = 1
        else:
            ln = (tag >> 2) + 1
            need = 2 if form == 2 else 4
        if ip + need > n:
            raise StreamError("truncated copy")
        if form == 1:
            off = ((tag >> 5) << 8) | stream[ip]
        else:
            off = int.from_bytes(stream[ip:ip + need], "little")
        ip += need
        if off == 0 or off > op + dict_size or op + ln > ulen:
            raise StreamError("bad copy")
        c["copy_tag%d" % (form if form < 3 else 3)] += 1
        if off > op:
            c["dict_only" if off - op >= ln else "dict_into_block"] += 1
        else:
            c["in_block"] += 1
            if off < ln and off <= 16:
                c["overlap_%d" % off] += 1
        op += ln
    if op != ulen:
        raise StreamError("short output")
    return c


REQUIRED_CLASSES = (["lit_ext%d" % i for i in range(5)]
                    + ["copy_tag1", "copy_tag2", "copy_tag3", "dict_only",
                       "dict_into_block", "in_block"]
                    + ["overlap_%d" % k for k in range(1, 17)])


# ------------------------------------------------------------------- corpus
def foreign_dictionary(seed=11) -> bytes:
    """The dictionary the foreign tests choose: 40 KiB of random bytes (far
    dict copies) ending in a tail the values quote."""
    rng = random.Random(seed)
    return rng.randbytes(40960) + b"<<dict-tail-0123456789>>"


def foreign_values(n, dictionary, seed=12):
    """n values that give the greedy encoder every copy class: slices of the
    dict (dict-only), the dict tail followed by the block head (a copy that
    starts in the dict and runs on into the block), repeats of earlier
    values (in-block), runs of period 1..16 (overlapping), random bytes."""
    rng = random.Random(seed)
    head = b"HEAD" + rng.randbytes(20)  # every block may start with it
    vals = []
    for i in range(n):
        kind = i % 8
        if kind == 0:
            v = head
        elif kind == 1:
            a = rng.randrange(0, len(dictionary) - 200)
            v = dictionary[a:a + rng.randint(8, 150)]
        elif kind == 2:
            v = rng.randbytes(3) + dictionary[-16:] + head[:16]
        elif kind == 3 and vals:
            v = rng.randbytes(2) + rng.choice(vals[-6:])[:80]
        elif kind == 4:
            k = 1 + (i // 8) % 16
            v = rng.randbytes(5) + rng.randbytes(k) * (40 // k + 3)
        elif kind == 5:
            v = rng.randbytes(rng.randint(0, 120))
        elif kind == 6:
            v = b""
        else:
            v = rng.randbytes(40) + dictionary[:64]
        vals.append(v)
    return vals


def ukey(i, width=16):
    return (b"k%0" + str(width - 1).encode() + b"d") % i


# --------------------------------------------------------- malformed inputs
def _one_block(z, stream, ulen=None, btype=2):
    """Replace value block 0's stored body; the index keeps its ulen."""
    z.vblocks[0][0] = btype
    z.vblocks[0][1] = bytes(stream)
    if ulen is not None:
        z.vblocks[0][2] = ulen


def _rec(U, sh, nonshared, tag, voff, vlen):
    return (_varint(sh) + _varint(len(nonshared)) + nonshared
            + struct.pack("<QII", tag, voff, vlen))


def _records(z, kb):
    """Decoded records of key block kb: [(ukey, tag, voff, vlen)]."""
    _, koff, ksize, _ = z.kblocks[kb]
    blk = bytes(z.key_area[koff:koff + ksize])
    out, p, prev = [], 0, b""
    while p < len(blk):
        sh, p = blk[p], p + 1  # U <= 48: one-byte varints
        ns, p = blk[p], p + 1
        key = prev[:sh] + blk[p:p + ns]
        p += ns
        tag, voff, vlen = struct.unpack_from("<QII", blk, p)
        p += 16
        out.append((key, tag, voff, vlen))
        prev = key
    return out


def _set_key_block(z, kb, body: bytes):
    """Replace key block kb's bytes (the last block, so no koff shifts)."""
    assert kb == len(z.kblocks) - 1
    koff = z.kblocks[kb][1]
    z.key_area = z.key_area[:koff] + bytearray(body)
    z.kblocks[kb][2] = len(body)


def _encode_records(U, recs, shared=None):
    out, prev = bytearray(), b""
    for i, (key, tag, voff, vlen) in enumerate(recs):
        sh = 0
        if i:
            while sh < U and sh < len(key) and key[sh] == prev[sh]:
                sh += 1
        if shared is not None and i in shared:
            sh = shared[i]
        out += _rec(U, sh, key[sh:], tag, voff, vlen)
        prev = key
    return bytes(out)


MALFORMED = (
    "copy_offset_0", "copy_offset_beyond_dict", "output_overrun",
    "truncated_op", "varint_len_ne_ulen", "literal_len_near_2_32",
    "unknown_btype", "shared_gt_U", "shared_plus_nonshared_ne_U",
    "records_65", "voff_vlen_past_block", "first_rank_not_monotone",
    "koff_ksize_past_key_area", "value_type_merge", "records_out_of_order",
    "flip_value_body", "flip_key_area", "flip_dict",
)


def malformed(data: bytes, name: str) -> bytes:
    """`data`: a good DZT file with >= 2 key blocks and >= 2 value blocks,
    16-byte keys.  Returns it damaged as `name` says; all but the flip_*
    cases sit behind valid checksums."""
    z = Dzt(data)
    U = z.U
    raw0 = z.raw_block(0)
    n0 = len(raw0)
    assert n0 >= 16 and len(z.kblocks) >= 2 and len(z.vblocks) >= 2
    pre = _varint(n0)
    lit = bytearray()
    emit_literal(lit, raw0[:8])
    last = len(z.kblocks) - 1
    recs = _records(z, last)
    if name == "copy_offset_0":
        s = bytearray(pre + lit)
        s += bytes([2 | (7 << 2), 0, 0])
        emit_literal(s, raw0[16:])
        _one_block(z, s)
    elif name == "copy_offset_beyond_dict":
        s = bytearray(pre + lit)
        emit_copy(s, len(z.dict) + 8 + 1, 8, 3)
        emit_literal(s, raw0[16:])
        _one_block(z, s)
    elif name == "output_overrun":
        s = bytearray(pre)
        emit_literal(s, raw0)
        emit_copy(s, 4, 8, 2)
        _one_block(z, s)
    elif name == "truncated_op":
        s = bytearray(pre)
        emit_literal(s, raw0[:n0 - 8])
        s += bytes([3 | (7 << 2), 8])  # 4-byte-offset copy, 1 offset byte
        _one_block(z, s)
    elif name == "varint_len_ne_ulen":
        s = bytearray(_varint(n0 - 1))
        emit_literal(s, raw0[:n0 - 1])
        _one_block(z, s)
    elif name == "literal_len_near_2_32":
        s = bytearray(pre)
        s += bytes([63 << 2]) + (0xFFFFFFFE).to_bytes(4, "little") + raw0
        _one_block(z, s)
    elif name == "unknown_btype":
        _one_block(z, encode(z.dict, raw0), btype=1)
    elif name == "shared_gt_U":
        body = bytearray(_encode_records(U, recs))
        first = len(_rec(U, 0, recs[0][0], 0, 0, 0))
        body[first] = U + 1  # second record's shared_u
        _set_key_block(z, last, bytes(body))
    elif name == "shared_plus_nonshared_ne_U":
        key, tag, voff, vlen = recs[0]
        body = _rec(U, 0, key + b"x", tag, voff, vlen) + \
            _encode_records(U, recs)[len(_rec(U, 0, key, tag, voff, vlen)):]
        _set_key_block(z, last, body)
    elif name == "records_65":
        # 65 records in the LAST block; n and the index follow, so only the
        # 64-record bound is broken
        key, tag, voff, vlen = recs[-1]
        seq = tag >> 8
        more = [(key, ((seq - 1 - i) << 8) | 1, voff, vlen)
                for i in range(65 - len(recs))]
        assert seq > 70
        _set_key_block(z, last, _encode_records(U, recs + more))
        z.n += len(more)
        struct.pack_into("<Q", z.props, 0, z.n)
    elif name == "voff_vlen_past_block":
        key, tag, voff, vlen = recs[-1]
        recs[-1] = (key, tag, z.vblocks[-1][2], 1)
        _set_key_block(z, last, _encode_records(U, recs))
    elif name == "first_rank_not_monotone":
        z.kblocks[1][3] = 0
    elif name == "koff_ksize_past_key_area":
        z.kblocks[last][2] += 1
    elif name == "value_type_merge":
        key, tag, voff, vlen = recs[-1]
        recs[-1] = (key, (tag & ~0xFF) | 2, voff, vlen)
        _set_key_block(z, last, _encode_records(U, recs))
    elif name == "records_out_of_order":
        assert len(recs) >= 3
        recs[-1], recs[-2] = recs[-2], recs[-1]
        _set_key_block(z, last, _encode_records(U, recs))
    elif name.startswith("flip_"):
        out = bytearray(data)
        dict_off, value_off = struct.unpack_from("<2Q", data, len(data) - FOOTER)
        assert value_off > dict_off > 8
        pos = {"flip_value_body": value_off + 3, "flip_key_area": 7,
               "flip_dict": dict_off + 1}[name]
        out[pos] ^= 0x40
        return bytes(out)
    else:
        raise KeyError(name)
    return z.build()


# ------------------------------------------------------ building DZT inputs
def oracle_dzt(tmp, name, entries, **kw):
    """entries: sorted [(internal_key, value)] -> the DZT file(s) the CPU
    oracle cuts from them (a one-run job with DZT output); returns paths.
    kw: oracle.make_job overrides (compression, checksum_type, snapshots,
    bottommost_level, target_file_size...)."""
    import os
    ct = kw.get("checksum_type", 4)
    src = os.path.join(str(tmp), name + ".src.sst")
    with open(src, "wb") as f:
        f.write(oracle.build_sst(
            entries, oracle.default_table_opts(checksum_type=ct)))
    out = os.path.join(str(tmp), name + ".dzt")
    os.makedirs(out)
    kw.setdefault("compression", 1)
    res = oracle.execute(oracle.make_job([[src]], out, output_table_factory=1,
                                         **kw))
    return [f["path"] for f in res["files"]]


def twin_sst(dzt_path, **opts) -> bytes:
    """The BlockBasedTable twin of a DZT file: same entry stream."""
    with open(dzt_path, "rb") as f:
        data = f.read()
    opts.setdefault("checksum_type", Dzt(data).ct)
    return oracle.build_sst(oracle.dzt_read(data),
                            oracle.default_table_opts(**opts))


def foreign_file(tmp, n=720):
    """One oracle-built DZT file over foreign_values (16-byte keys)."""
    d = foreign_dictionary()
    vals = foreign_values(n, d)
    entries = [(oracle.make_ikey(ukey(i), 1000 + i, 1), v)
               for i, v in enumerate(vals)]
    (path,) = oracle_dzt(tmp, "foreign", entries, bottommost_level=0)
    return path, d
