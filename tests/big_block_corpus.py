"""Shared inputs of the large-block tests (data blocks over 16 KiB with
snappy output): the value shapes, the block-size ladder and a reader for the
data-block handles of a finished SST.  The CPU test feeds these bytes to
tools/enc_big_host, the GPU test runs jobs over the same values.
Everything is seeded; nothing here touches the GPU.
"""
import functools
import random
import struct

import oracle

TYPE_DELETION, TYPE_VALUE = 0, 1
SNAP_MAX_UNC = 16384  # dcw_k_emit.h: larger blocks go to k_compress_large

# Data-block sizes of the ladder: 16384 and below is the default kernel,
# 16385 the first block of the large one; from 65536 on a copy may need the
# 4-byte-offset form, and 65539 is the first size whose last hashed position
# (n - 4) no longer fits below a u16 table's 0xffff sentinel.
LADDER = (16383, 16384, 16385, 16386, 65538, 65539, 65540, 65600)


def k16(i):
    return b"key%013d" % i  # 16-byte user keys: the worker's fast key path


def periodic(n, seed, period=97):
    """n compressible bytes of a period that is no power of two."""
    pat = random.Random(seed).randbytes(period)
    return (pat * (n // period + 1))[:n]


def _varint_len(v):
    n = 1
    while v >= 0x80:
        v >>= 7
        n += 1
    return n


def value_len_for_block(block_bytes, klen=24):
    """Value length that makes a one-entry data block of block_bytes: shared
    and non-shared varints (1 + 1), the value-length varint, the internal
    key, the value, one restart and the footer (4 + 4)."""
    for vlen in (block_bytes - 2 - klen - 8 - k for k in (1, 2, 3, 4)):
        if 2 + _varint_len(vlen) + klen + vlen + 8 == block_bytes:
            return vlen
    raise AssertionError(block_bytes)


@functools.lru_cache(maxsize=None)
def shapes():
    """name -> value.  The four shapes of the issue's table."""
    rng = random.Random(0xB16)
    head = rng.randbytes(1000)
    twenty = rng.randbytes(20000)
    return {
        # 2-byte offsets up to position 65536 + 97, 4-byte offsets behind it
        "periodic70k": periodic(70810, 0xB17),
        # long literals, then 130 copies of the head at offsets up to 200000
        "far201k": head + rng.randbytes(70000) + head * 130,
        # fails the 896/1024 ratio: stored raw, pass 2 skipped
        "random20k": rng.randbytes(20000),
        # second half copies the first: accepted at about 0.72
        "random20k_twice": twenty + twenty,
    }


def _get_varint(b, i):
    r, sh = 0, 0
    while True:
        x = b[i]
        i += 1
        r |= (x & 0x7F) << sh
        if not x & 0x80:
            return r, i
        sh += 7


def data_blocks(sst):
    """-> [(offset, stored size, block type, uncompressed size)] of the data
    blocks of a format_version 5 SST, read from its index block (restart
    interval 1: every index value is a full handle)."""
    f = sst[-53:]
    assert struct.unpack("<I", f[41:45])[0] == 5
    _, i = _get_varint(f, 1)
    _, i = _get_varint(f, i)
    idx_off, i = _get_varint(f, i)
    idx_sz, i = _get_varint(f, i)
    idx = sst[idx_off:idx_off + idx_sz]
    if sst[idx_off + idx_sz] == 1:
        idx = oracle.snappy_uncompress(idx)
    nres = struct.unpack("<I", idx[-4:])[0] & 0x7FFFFFFF
    end = len(idx) - 4 - 4 * nres
    out, p = [], 0
    while p < end:
        shared, p = _get_varint(idx, p)
        ns, p = _get_varint(idx, p)
        assert shared == 0
        p += ns
        off, p = _get_varint(idx, p)
        sz, p = _get_varint(idx, p)
        btype = sst[off + sz]
        unc = _get_varint(sst, off)[0] if btype == 1 else sz
        out.append((off, sz, btype, unc))
    return out


def ikey_sort(kvs):
    return sorted(kvs, key=lambda e: (e[0], -((e[1] << 8) | e[2])))


def write_run(directory, name, kvs, **table_opts):
    """kvs: [(user key, seq, type, value)] -> path of an input SST."""
    es = [(oracle.make_ikey(k, s, t), v) for k, s, t, v in ikey_sort(kvs)]
    p = str(directory / name)
    opts = oracle.default_table_opts(**table_opts) if table_opts else None
    with open(p, "wb") as f:
        f.write(oracle.build_sst(es, opts))
    return p
