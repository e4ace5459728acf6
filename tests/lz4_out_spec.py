"""The LZ4 output codec ("DCW LZ4 codec v1", toplingdb_amd/csrc/dcw_lz4_enc.h)
in plain Python: which matches the encoder takes.  The stream is then
foreign_lz4.emit of exactly those matches; every C++ form must agree."""
import random

from foreign_lz4 import decode, emit, frame, unframe  # noqa: F401

WINDOW, HASH_BITS, HASH_MUL = 65536, 11, 0x1e35a7bd


def matches(raw):
    """-> [(position, offset, length)] in position order"""
    n, out = len(raw), []

    def h(p):
        return (int.from_bytes(raw[p:p + 4], "little") * HASH_MUL
                & 0xffffffff) >> (32 - HASH_BITS)

    for base in range(0, n, WINDOW):
        end = min(base + WINDOW, n)
        tab = {}
        for p in range(base, end - 3):  # the smallest position per slot
            tab.setdefault(h(p), p)
        seg = max(16, (end - base + 63) // 64)
        for s0 in range(base, end, seg):
            s1, p = min(s0 + seg, end), s0
            while p + 4 <= s1 and p + 12 <= n:
                c = tab[h(p)]
                if c < p and raw[c:c + 4] == raw[p:p + 4]:
                    ln = 4
                    while p + ln < min(s1, n - 5) and raw[c + ln] == raw[p + ln]:
                        ln += 1
                    out.append((p, p - c, ln))
                    p += ln
                else:
                    p += 1
    return out


def encode(raw):
    """-> the stored payload of a type-4/5 block, or None: stored raw"""
    payload = frame(emit(raw, matches(raw)), len(raw))
    return payload if len(payload) <= (896 * len(raw)) >> 10 else None


def seam_block():
    """4096 bytes, seg = 64: an 8-byte word repeats after random stretches
    (the first leaves lane 0 without a match), then back to back"""
    rng = random.Random(0x5EA)
    word = rng.randbytes(8)
    buf = word + b"".join(rng.randbytes(g) + word for g in (
        62, 14, 15, 16, 269, 270, 271, 130, 165, 400))
    buf += word * ((4056 - len(buf)) // 8)
    return buf + rng.randbytes(4096 - len(buf))


MATCH_LENGTHS = (4, 18, 19, 20, 273, 274)


def match_length_block():
    """65536 random bytes, seg = 1024: a prefix of the block of each length
    in MATCH_LENGTHS, in a lane of its own"""
    rng = random.Random(0x3A7)
    buf = bytearray(rng.randbytes(65536))
    for i, ml in enumerate(MATCH_LENGTHS):
        at = 1024 * (i + 1) + 100
        buf[at:at + ml + 1] = buf[:ml] + bytes([buf[ml] ^ 0xff])
    return bytes(buf)
