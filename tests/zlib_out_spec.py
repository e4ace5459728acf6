"""The zlib output codec ("DCW deflate codec v1",
toplingdb_amd/csrc/dcw_deflate_enc.h) in plain Python: matches, code lengths,
header, emit, accept.  Every C++ form must give these bytes."""
import random

from foreign_lz4 import frame
from foreign_zlib import huff, pack

WINDOW, HASH_BITS, HASH_MUL = 16384, 11, 0x1e35a7bd
LEN_EXTRA = [0] * 8 + [e for e in range(1, 6) for _ in range(4)] + [0]
LEN_BASE = [3 + sum(1 << e for e in LEN_EXTRA[:i]) for i in range(28)] + [258]
DIST_EXTRA = [0, 0] + [e for e in range(14) for _ in range(2)]
DIST_BASE = [1 + sum(1 << e for e in DIST_EXTRA[:i]) for i in range(30)]
CL_LEN = [4, 5, 6, 6, 5, 5, 4, 3, 3, 3, 4, 4, 5, 5, 6, 6, 5, 4, 4]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def window_symbols(raw, base, end):
    """-> the window's symbols in position order: a byte, or (length, distance)"""
    def h(p):
        return (int.from_bytes(raw[p:p + 4], "little") * HASH_MUL
                & 0xffffffff) >> (32 - HASH_BITS)

    tab, out = {}, []
    for p in range(base, end - 3):  # the smallest position per slot
        tab.setdefault(h(p), p)
    seg = max(16, (end - base + 63) // 64)
    for s0 in range(base, end, seg):
        s1, p = min(s0 + seg, end), s0
        while p < s1:
            c = tab[h(p)] if p + 4 <= s1 else p
            if c < p and raw[c:c + 4] == raw[p:p + 4]:
                ln = 4
                while p + ln < s1 and raw[c + ln] == raw[p + ln]:
                    ln += 1
                out.append((ln, p - c))
                p += ln
            else:
                out.append(raw[p])
                p += 1
    return out


def classify(value, base):
    s = max(i for i, b in enumerate(base) if b <= value)
    return s, value - base[s]


def code_lengths(freq):
    """Shannon lengths, then shortened in (f descending, symbol ascending)
    passes until the Kraft sum is exactly one"""
    order = sorted((s for s, f in enumerate(freq) if f), key=lambda s: (-freq[s], s))
    lens, total = [0] * len(freq), sum(freq)
    for s in order:
        lens[s] = next(L for L in range(1, 16) if freq[s] << L >= total)
    slack = (1 << 15) - sum(1 << (15 - lens[s]) for s in order)
    while len(order) >= 2 and slack > 0:
        for s in order:
            gain = 1 << (15 - lens[s])
            if lens[s] > 1 and gain <= slack:
                lens[s] -= 1
                slack -= gain
    return lens


def canonical(lens):
    """-> symbol -> (value, nbits) of the bit writer"""
    out, code = {}, 0
    for nbits in range(1, 16):
        for s, ln in enumerate(lens):
            if ln == nbits:
                out[s] = huff(code, nbits)
                code += 1
        code <<= 1
    return out


def header_fields(seq):
    """the code-length symbols of the HLIT + HDIST lengths, greedy"""
    cl, out, i = canonical(CL_LEN), [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 11:
            take = min(r, 138)
            out += [cl[18], (take - 11, 7)]
        elif v == 0 and r >= 3:
            take = r
            out += [cl[17], (take - 3, 3)]
        elif v and i and seq[i - 1] == v and r >= 3:
            take = min(r, 6)
            out += [cl[16], (take - 3, 2)]
        else:
            take = 1
            out.append(cl[v])
        i += take
    return out


def window_fields(symbols, final):
    """-> the window's deflate block as (value, nbits) fields, and its form"""
    fl, fd, coded = [0] * 286, [0] * 30, []
    fl[256] = 1
    for s in symbols:
        if isinstance(s, tuple):
            ls, dsym = classify(s[0], LEN_BASE), classify(s[1], DIST_BASE)
            fl[257 + ls[0]] += 1
            fd[dsym[0]] += 1
            coded.append((257 + ls[0], (ls[1], LEN_EXTRA[ls[0]]),
                          dsym[0], (dsym[1], DIST_EXTRA[dsym[0]])))
        else:
            fl[s] += 1
            coded.append((s,))
    coded.append((256,))
    ll, dl = code_lengths(fl), code_lengths(fd)
    hlit = max(s for s in range(286) if fl[s]) + 1
    hdist = max([s for s in range(30) if fd[s]] + [0]) + 1
    head = [(final, 1), (2, 2), (hlit - 257, 5), (hdist - 1, 5), (15, 4)]
    head += [(CL_LEN[s], 3) for s in CL_ORDER] + header_fields(ll[:hlit] + dl[:hdist])

    def body(lcode, dcode):
        out = []
        for c in coded:
            out.append(lcode[c[0]])
            if len(c) > 1:
                out += [c[1], dcode[c[2]], c[3]]
        return out

    dyn = head + body(canonical(ll), canonical(dl))
    fix = [(final, 1), (1, 2)] + body(canonical(FIXED), canonical([5] * 30))
    bits = [sum(n for _, n in f) for f in (dyn, fix)]
    return (dyn, "dynamic") if bits[0] < bits[1] else (fix, "fixed")


def stream(raw):
    """-> (stored payload, form of each window, largest distance)"""
    fields, forms, far = [], [], 0
    for base in range(0, len(raw), WINDOW):
        end = min(base + WINDOW, len(raw))
        symbols = window_symbols(raw, base, end)
        far = max([far] + [s[1] for s in symbols if isinstance(s, tuple)])
        f, form = window_fields(symbols, int(end == len(raw)))
        fields += f
        forms.append(form)
    return frame(pack(fields), len(raw)), forms, far


def encode(raw):
    """-> the stored payload of a type-2 block, or None: stored raw"""
    payload = stream(raw)[0]
    return payload if len(payload) <= (896 * len(raw)) >> 10 else None


LENGTH_EDGES = (4, 10, 11, 18, 19, 34, 35, 66, 67, 130, 131, 256)
DISTANCE_EDGES = sorted({1} | {d for b in DIST_BASE[1:28] for d in (b - 1, b)})


def boundary_block():
    """16384 random bytes, seg = 256.  Source j, 8 bytes at 21*j + 8, comes
    again DISTANCE_EDGES[j] later (a distance below 8 as a period); lanes
    46..57 begin with the block's first bytes, one of LENGTH_EDGES each.  A
    source is found where no earlier position has its hash: the seed's doing."""
    rng = random.Random(0xB3)
    buf = bytearray(rng.randbytes(16384))
    for j, d in enumerate(DISTANCE_EDGES):
        c = 21 * j + 8
        if d < 8:
            buf[c:c + d + 8] = (buf[c:c + d] * 16)[:d + 8]
        else:
            buf[c + d:c + d + 9] = buf[c:c + 8] + bytes([buf[c + 8] ^ 0xff])
    for i, ln in enumerate(LENGTH_EDGES):
        at = 256 * (46 + i)
        buf[at:at + ln + 1] = buf[:ln] + bytes([buf[ln] ^ 0xff])
    return bytes(buf[:16384])


def three_window_block():
    """one block of three windows: six-bit bytes without a match (the seed's
    doing); 1024 bytes twice, then random bytes (every match at distance
    1024: one distance symbol); 1024 bytes twice, then 2048 bytes twice (two)"""
    rng = random.Random(0x4B)
    six = bytes(rng.choices(range(48, 112), k=16384))
    a, b = rng.randbytes(1024), rng.randbytes(2048)
    return six + a * 2 + rng.randbytes(14336) + a * 2 + b * 2 + rng.randbytes(200)
