// dcw_deflate_enc.h — the deflate (RFC 1951) encoder for output data blocks
// of type 2 (kZlibCompression).  Plain C++ shared by k_compress_zlib
// (dcw_zlib_enc.hip), dcw_host.cpp and the host check program
// (tools/zlib_enc_host).  The decoder is dcw_inflate_dec.h.
//
// "DCW deflate codec v1" (self-pinned like the snappy and LZ4 codecs,
// SURVEY.md §8c; any inflate with a window of 16 KiB or more reads it).  A
// stored block is varint32(n) + one raw deflate stream, a pure function of
// the block's bytes in[0, n):
//   windows   [w*16384, min((w+1)*16384, n)); one deflate block per window,
//             BFINAL on the last, never a stored block; matches are found
//             inside a window only, so every distance is <= 16383
//   table     per window, 1 << kSnapHashBits slots, the snappy codec's hash;
//             a slot holds the SMALLEST position p of the window, p + 4 <=
//             window end, with that hash (order-independent)
//   segments  per window, seg = snap_segment_size(window length) <= 256; lane
//             i owns [base + i*seg, min(base + (i+1)*seg, window end))
//   walk      of a segment [s0, s1): p = s0; while p + 4 <= s1: candidate c =
//             tab[h(p)] matches if c < p and load32(c) == load32(p); the
//             match is extended while p + l < s1; p += l, else in[p] is a
//             literal and p += 1.  The bytes left over are literals.  A match
//             lies inside its segment, so its length is 4..256: deflate's 258
//             is never reached, no length cap is needed and length symbol 285
//             is never written.  Deflate has no end rules; the only bound is
//             that the 4-byte loads stay inside the segment
//   symbols   of a window: the literals and (length, distance) pairs of all
//             segments in position order, then symbol 256.  A symbol belongs
//             to one segment
//   counts    f[0, 286) of the literal/length symbols, 256 counted once, and
//             f[0, 30) of the distance symbols
//   lengths   per alphabet, of the symbols with f > 0, T their sum: start
//             from the smallest L >= 1 with f << L >= T (Shannon's length; at
//             most 15 because T <= 16385; the Kraft sum is then <= 1).  Let
//             slack = 2^15 - sum 2^(15 - L).  While slack > 0, pass over the
//             symbols in the order (f descending, symbol ascending): a symbol
//             with L > 1 and 2^(15 - L) <= slack takes L - 1, and slack drops
//             by that 2^(15 - L).  Every pass shortens a longest code, so the
//             passes end with a complete code of at most 15 bits.  Integer
//             arithmetic only.  Two exceptions for the distance alphabet: no
//             symbol at all is written as one distance length of 0 (HDIST
//             field 0), a single symbol gets length 1 (the rule's start, no
//             pass); zlib and dcw_inflate_dec.h accept both
//   header    dynamic form: HLIT = 1 + the highest literal/length symbol with
//             f > 0, HDIST likewise (at least 1), HCLEN = 19.  The
//             code-length code is one constant complete code, by symbol 0..18
//             of the lengths 4 5 6 6 5 5 4 3 3 3 4 4 5 5 6 6 5 4 4.  The HLIT
//             + HDIST lengths are one sequence; at position i with value v
//             and r equal values from i on: v = 0: r >= 11 writes 18 for
//             min(r, 138), r >= 3 writes 17 for r, else a 0; v != 0: if the
//             value before i is v too and r >= 3, 16 for min(r, 6), else v
//   form      the exact bit count of the dynamic form, header included, and
//             of the fixed form (BTYPE 1) are compared; the smaller is
//             written, the fixed one on a tie
//   accept    stored compressed iff preamble + ceil(bits / 8) <= (896*n) >> 10;
//             the padding bits of the last byte are zero
//
// Canonical codes are assigned as RFC 1951 3.2.2 says and held bit-reversed:
// deflate packs a Huffman code most significant bit first into a stream
// that is filled from the least significant bit.
//
// deflate_encode_block is the serial restatement.  The wave form below it
// (DCW_DEFLATE_WAVE) is what the kernel runs, one wave per block; the check
// program runs the same text with the lanes in a loop.
#pragma once
#include "dcw_common.h"

namespace dcw {

static const uint32_t kDeflWindow = 16384;
static const uint32_t kDeflMaxUnc = 0x7fffffffu; // as the LZ4 encoder's bound
// one array holds both alphabets: literal/length at 0, distance at kDeflD0
static const uint32_t kDeflD0 = 288, kDeflSyms = 320;

// A literal costs at most 9 bits and a match less than its bytes as literals
// (fixed form, never undercut by the form that is written); a window adds
// its 3 header bits and at most 7 for symbol 256.
DCW_HD size_t deflate_max_compressed(size_t n) {
  return n + n / 8 + (n >> 12) + 16;
}

// length 3..257 and distance 1..32768 to symbol, extra-bit count and value
DCW_HD uint32_t defl_len_sym(uint32_t l, uint32_t* eb, uint32_t* ev) {
  uint32_t v = l - 3;
  uint32_t e = v < 8 ? 0 : 29 - (uint32_t)__builtin_clz(v);
  *eb = e;
  *ev = v & ((1u << e) - 1);
  return v < 8 ? 257 + v : 261 + 4 * e + ((v >> e) & 3);
}
DCW_HD uint32_t defl_dist_sym(uint32_t d, uint32_t* eb, uint32_t* ev) {
  uint32_t v = d - 1;
  uint32_t hb = v < 4 ? 1 : 31 - (uint32_t)__builtin_clz(v);
  *eb = hb - 1;
  *ev = v & ((1u << (hb - 1)) - 1);
  return v < 4 ? v : 2 * hb + ((v >> (hb - 1)) & 1);
}
// extra bits and fixed-form length of entry i of the joint array
DCW_HD uint32_t defl_extra(uint32_t i) {
  if (i < 265 || i == 285) return 0;
  if (i < kDeflD0) return (i - 261) >> 2;
  return i < kDeflD0 + 4 ? 0 : ((i - kDeflD0) >> 1) - 1;
}
DCW_HD uint32_t defl_fixed_len(uint32_t i) {
  return i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < kDeflD0 ? 8 : 5;
}
DCW_HD uint32_t defl_rev(uint32_t code, uint32_t len) {
  uint32_t r = 0;
  for (uint32_t t = 0; t < len; t++, code >>= 1) r = (r << 1) | (code & 1);
  return r;
}
// the constant code-length code: length of symbol s, three bits each
DCW_HD uint32_t defl_cl_len(uint32_t s) {
  const uint64_t lens = 4ull | 5ull << 3 | 6ull << 6 | 6ull << 9 | 5ull << 12 |
                        5ull << 15 | 4ull << 18 | 3ull << 21 | 3ull << 24 |
                        3ull << 27 | 4ull << 30 | 4ull << 33 | 5ull << 36 |
                        5ull << 39 | 6ull << 42 | 6ull << 45 | 5ull << 48 |
                        4ull << 51 | 4ull << 54;
  return (uint32_t)(lens >> (3 * s)) & 7;
}
DCW_HD uint32_t defl_cl_code(uint32_t s) { // canonical, bit-reversed
  uint32_t len = defl_cl_len(s), code = 0;
  for (uint32_t t = 0; t < 19; t++) {
    uint32_t lt = defl_cl_len(t);
    if (lt < len) code += 1u << (len - lt);
    if (lt == len && t < s) code++;
  }
  return defl_rev(code, len);
}
// the symbol whose length is the i-th of the header: 16 17 18 0 8 7 9 6 10 5
// 11 4 12 3 13 2 14 1 15
DCW_HD uint32_t defl_cl_order(uint32_t i) {
  if (i < 3) return 16 + i;
  if (i == 3) return 0;
  return (i & 1) ? 9 - (i >> 1) : 6 + (i >> 1);
}

// entry j of the header's length sequence: hlit literal/length lengths, then
// the distance lengths
DCW_HD uint32_t defl_seq(const uint8_t* len, uint32_t hlit, uint32_t j) {
  return j < hlit ? len[j] : len[kDeflD0 + (j - hlit)];
}
// What the header rule writes at position i of `tot`: a code-length symbol
// with its extra bits, or sym = 19 where an earlier repeat covers i.  A pure
// function of i's run of equal values, so every position can be asked alone.
struct DeflTok {
  uint32_t sym, eb, ev;
};
DCW_HD DeflTok defl_hdr_token(const uint8_t* len, uint32_t hlit, uint32_t tot,
                              uint32_t i) {
  uint32_t v = defl_seq(len, hlit, i), a = i, b = i + 1;
  while (a > 0 && defl_seq(len, hlit, a - 1) == v) a--;
  while (b < tot && defl_seq(len, hlit, b) == v) b++;
  uint32_t k = i - a, run = b - a, chunk = 138;
  DeflTok t = {v, 0, 0};
  if (v) { // the run's first value is written out, repeats come in sixes
    if (k == 0) return t;
    k--;
    run--;
    chunk = 6;
  }
  uint32_t c = k - k % chunk, left = run - c; // at the start of i's chunk
  if (left < 3) return t;
  uint32_t take = left < chunk ? left : chunk;
  if (k != c) t = {19, 0, 0};
  else if (v) t = {16, 2, take - 3};
  else if (take >= 11) t = {18, 7, take - 11};
  else t = {17, 3, take - 3};
  return t;
}

// The walk of one segment [s0, s1) of the window at `base`; tab holds
// window-relative positions.  f.lit(byte) and f.match(length, distance) are
// called in position order.  Loads stay below s1: a candidate lies below p,
// and a load at c + l is paired with one at p + l.  An empty slot (0xffff)
// lies above every p of the window.
template <class F>
DCW_HD void defl_walk(const uint8_t* __restrict__ in, uint32_t base, uint32_t s0,
                      uint32_t s1, const uint16_t* __restrict__ tab, F& f) {
  uint32_t p = s0;
  while (p + 4 <= s1) {
    uint32_t w = load32(in + p);
    uint32_t c = base + tab[(w * kSnapHashMul) >> (32 - kSnapHashBits)];
    if (c >= p || load32(in + c) != w) {
      f.lit(w & 0xffu);
      p++;
      continue;
    }
    uint32_t l = 4;
    while (p + l + 4 <= s1) {
      uint32_t x = load32(in + c + l) ^ load32(in + p + l);
      if (x) break;
      l += 4;
    }
    while (p + l < s1 && in[c + l] == in[p + l]) l++;
    f.match(l, p - c);
    p += l;
  }
  for (; p < s1; p++) f.lit(in[p]);
}

// ------------------------------------------------------ serial restatement
struct DeflSerialBits { // a bit writer, least significant bit first
  uint8_t* out;
  uint64_t at; // bits written
  void put(uint32_t v, uint32_t nb) {
    for (uint32_t t = 0; t < nb; t++, at++) {
      if ((at & 7) == 0) out[at >> 3] = 0;
      out[at >> 3] |= (uint8_t)(((v >> t) & 1) << (at & 7));
    }
  }
};
struct DeflSerialCount {
  uint32_t* f;
  void lit(uint32_t b) { f[b]++; }
  void match(uint32_t l, uint32_t d) {
    uint32_t eb, ev;
    f[defl_len_sym(l, &eb, &ev)]++;
    f[kDeflD0 + defl_dist_sym(d, &eb, &ev)]++;
  }
};
struct DeflSerialEmit {
  DeflSerialBits* w;
  const uint8_t* len;
  const uint16_t* code;
  void sym(uint32_t s, uint32_t eb, uint32_t ev) {
    w->put(code[s], len[s]);
    w->put(ev, eb);
  }
  void lit(uint32_t b) { sym(b, 0, 0); }
  void match(uint32_t l, uint32_t d) {
    uint32_t eb, ev, s = defl_len_sym(l, &eb, &ev);
    sym(s, eb, ev);
    s = kDeflD0 + defl_dist_sym(d, &eb, &ev);
    sym(s, eb, ev);
  }
};
// the length rule over f[0, nsym), as the header comment states it
inline void defl_serial_lengths(const uint32_t* f, uint32_t nsym, uint8_t* len) {
  uint32_t order[kDeflD0], used = 0, total = 0, slack = 1u << 15;
  for (uint32_t s = 0; s < nsym; s++) {
    len[s] = 0;
    if (f[s] == 0) continue;
    uint32_t at = used++; // insertion: f descending, symbol ascending
    for (; at > 0 && f[order[at - 1]] < f[s]; at--) order[at] = order[at - 1];
    order[at] = s;
    total += f[s];
  }
  for (uint32_t k = 0; k < used; k++) {
    uint32_t s = order[k];
    for (len[s] = 1; (f[s] << len[s]) < total;) len[s]++;
    slack -= 1u << (15 - len[s]);
  }
  while (used >= 2 && slack > 0)
    for (uint32_t k = 0; k < used; k++) {
      uint32_t s = order[k], gain = 1u << (15 - len[s]);
      if (len[s] > 1 && gain <= slack) {
        len[s]--;
        slack -= gain;
      }
    }
}
inline void defl_serial_codes(const uint8_t* len, uint32_t nsym, uint16_t* code) {
  uint32_t count[16] = {0}, next[16] = {0};
  for (uint32_t s = 0; s < nsym; s++) count[len[s]]++;
  count[0] = 0;
  for (uint32_t l = 1; l < 16; l++) next[l] = (next[l - 1] + count[l - 1]) << 1;
  for (uint32_t s = 0; s < nsym; s++)
    if (len[s]) code[s] = (uint16_t)defl_rev(next[len[s]]++, len[s]);
}

// Writes varint32(n) + the stream, at most 5 + deflate_max_compressed(n)
// bytes, and returns their count.  0 < n <= kDeflMaxUnc.
inline size_t deflate_encode_block(const uint8_t* in, uint32_t n, uint8_t* out) {
  DeflSerialBits w = {out, 8 * (uint64_t)varint32_put(out, n)};
  uint16_t tab[1u << kSnapHashBits], code[kDeflSyms];
  uint32_t f[kDeflSyms];
  uint8_t len[kDeflSyms];
  for (uint32_t base = 0; base < n; base += kDeflWindow) {
    uint32_t wend = n - base > kDeflWindow ? base + kDeflWindow : n;
    for (uint32_t t = 0; t < (1u << kSnapHashBits); t++) tab[t] = 0xffffu;
    for (uint32_t p = base; p + 4 <= wend; p++) {
      uint32_t h = (load32(in + p) * kSnapHashMul) >> (32 - kSnapHashBits);
      if (tab[h] == 0xffffu) tab[h] = (uint16_t)(p - base);
    }
    uint32_t seg = (uint32_t)snap_segment_size(wend - base);
    for (uint32_t i = 0; i < kDeflSyms; i++) f[i] = 0;
    DeflSerialCount count = {f};
    for (uint32_t s0 = base; s0 < wend; s0 += seg)
      defl_walk(in, base, s0, wend - s0 > seg ? s0 + seg : wend, tab, count);
    f[256] = 1;
    defl_serial_lengths(f, 286, len);
    defl_serial_lengths(f + kDeflD0, 30, len + kDeflD0);
    len[286] = len[287] = len[kDeflD0 + 30] = len[kDeflD0 + 31] = 0;
    uint32_t hlit = 257, hdist = 1;
    for (uint32_t s = 257; s < 286; s++)
      if (f[s]) hlit = s + 1;
    for (uint32_t s = 1; s < 30; s++)
      if (f[kDeflD0 + s]) hdist = s + 1;
    // the header's symbols, by the rule in its serial form
    uint32_t tot = hlit + hdist, ntok = 0;
    DeflTok tok[kDeflSyms];
    for (uint32_t i = 0; i < tot;) {
      uint32_t v = defl_seq(len, hlit, i), r = 1;
      while (i + r < tot && defl_seq(len, hlit, i + r) == v) r++;
      DeflTok t = {v, 0, 0};
      uint32_t take = 1;
      if (v == 0 && r >= 11) {
        take = r < 138 ? r : 138;
        t = {18, 7, take - 11};
      } else if (v == 0 && r >= 3) {
        take = r;
        t = {17, 3, take - 3};
      } else if (v && i > 0 && defl_seq(len, hlit, i - 1) == v && r >= 3) {
        take = r < 6 ? r : 6;
        t = {16, 2, take - 3};
      }
      tok[ntok++] = t;
      i += take;
    }
    uint64_t dyn = 3 + 14 + 57, fix = 3;
    for (uint32_t k = 0; k < ntok; k++) dyn += defl_cl_len(tok[k].sym) + tok[k].eb;
    for (uint32_t i = 0; i < kDeflSyms; i++) {
      dyn += (uint64_t)f[i] * (len[i] + defl_extra(i));
      fix += (uint64_t)f[i] * (defl_fixed_len(i) + defl_extra(i));
    }
    w.put(wend == n ? 1 : 0, 1);
    if (dyn < fix) {
      w.put(2, 2);
      w.put(hlit - 257, 5);
      w.put(hdist - 1, 5);
      w.put(15, 4);
      for (uint32_t i = 0; i < 19; i++) w.put(defl_cl_len(defl_cl_order(i)), 3);
      for (uint32_t k = 0; k < ntok; k++) {
        w.put(defl_cl_code(tok[k].sym), defl_cl_len(tok[k].sym));
        w.put(tok[k].ev, tok[k].eb);
      }
    } else {
      w.put(1, 2);
      for (uint32_t i = 0; i < kDeflSyms; i++)
        len[i] = (uint8_t)(i < kDeflD0 + 30 ? defl_fixed_len(i) : 0);
    }
    defl_serial_codes(len, kDeflD0, code);
    defl_serial_codes(len + kDeflD0, 32, code + kDeflD0);
    DeflSerialEmit emit = {&w, len, code};
    for (uint32_t s0 = base; s0 < wend; s0 += seg)
      defl_walk(in, base, s0, wend - s0 > seg ? s0 + seg : wend, tab, emit);
    emit.sym(256, 0, 0);
  }
  return (size_t)((w.at + 7) >> 3);
}

#ifdef DCW_DEFLATE_WAVE
// ---------------------------------------------------------------- wave form
// One wave encodes one block.  As in dcw_inflate_dec.h the code is a sequence
// of phases: `DW_LANES { ... }` is the body one lane runs (on the host a loop
// over the 64 lanes, ascending or descending), DW_SYNC() separates phases
// that communicate through DeflLds or the output.  What stands between the
// phases is lane-uniform: it depends on DeflLds fields read after a sync.
// Counters are integer LDS atomics, order-independent.
//
// Per window (defl_wave_code): the min-position table; the walk that counts
// symbols; Shannon lengths and each symbol's rank in (f descending, symbol
// ascending), the lanes taking the 320 entries in turn; the passes of the
// length rule in class form: ranks of one length are consecutive and lengths
// do not fall along the order, so a pass shortens, for L = 2..15 in turn,
// the first min(count[L], slack >> (15 - L)) symbols of length L, which every
// symbol works out for itself from the 15 class counts; then the header's
// symbols, five positions per lane, and both forms' bit counts.
// Per window again, once the block is accepted (defl_wave_emit): canonical
// codes (lane L - 1 numbers the symbols of length L); a walk that measures
// each lane's bits and their prefix sum; the header; the walk that writes.
//
// Bits meet inside a word at every seam between lanes, between header and
// symbols and between windows.  No two lanes ever write the same global
// word: of the words a lane touches, those that hold one of the 65 lane
// boundaries of the window are gathered in DeflLds::stage by LDS OR (the slot
// of a word is the first boundary in it), the header in DeflLds::hstage, and
// whole words are stored after a sync; words inside a lane's range go
// straight to the output.  The window's last, partial word is handed to the
// next window's header as `carry`, and stored by defl_enc_wave at the end.
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
#define DFN __device__ __forceinline__
#define DMF __device__ __forceinline__ // a member function
#define DW_LANES for (uint32_t lane = zlane, dwonce = 1; dwonce; dwonce = 0)
#define DW_SYNC()                                          \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); \
    __builtin_amdgcn_s_waitcnt(0);                         \
    __builtin_amdgcn_wave_barrier();                       \
  } while (0)
#define DW_ADD(p, v) ((void)atomicAdd((p), (v)))
#define DW_OR(p, v) ((void)atomicOr((p), (v)))
#define DW_MAX(p, v) ((void)atomicMax((p), (v)))
// min into a u16 slot: CAS on the aligned u32 around it
DFN void dw_min16(uint16_t* tab, uint32_t h, uint32_t p) {
  uint32_t* w = (uint32_t*)tab + (h >> 1);
  uint32_t sh = (h & 1u) * 16;
  uint32_t old = *(volatile uint32_t*)w;
  for (;;) {
    if (p >= ((old >> sh) & 0xffffu)) return;
    uint32_t got = atomicCAS(w, old, (old & ~(0xffffu << sh)) | (p << sh));
    if (got == old) return;
    old = got;
  }
}
#else
#define DFN static inline
#define DMF inline
static int dw_descending = 0; // the host runs every block in both lane orders
#define DW_LANES \
  for (uint32_t ii = 0, lane = dw_descending ? 63 : 0; ii < 64; \
       ii++, lane = dw_descending ? 63 - ii : ii)
#define DW_SYNC() ((void)0)
#define DW_ADD(p, v) (*(p) += (v))
#define DW_OR(p, v) (*(p) |= (v))
#define DW_MAX(p, v) (*(p) = *(p) < (v) ? (v) : *(p))
DFN void dw_min16(uint16_t* tab, uint32_t h, uint32_t p) {
  if (p < tab[h]) tab[h] = (uint16_t)p;
}
#endif

struct alignas(16) DeflLds {
  uint16_t tab[1u << kSnapHashBits];
  uint32_t f[kDeflSyms];     // counts
  uint16_t code[kDeflSyms];  // bit-reversed codes
  uint16_t rank[kDeflSyms];  // place in (f descending, symbol ascending)
  uint8_t len[kDeflSyms];
  uint32_t cnt[2][2][16];    // [buffer][alphabet][length]: symbols per length
  uint32_t tot[2], top[2];   // per alphabet: sum of f, 1 + highest used symbol
  uint32_t sum[2];           // bits of the dynamic and of the fixed form
  uint32_t hcost[64];        // header bits of a lane's five positions
  uint32_t lraw[64];         // symbol bits of a lane's segment
  uint32_t lbits[65];        // their exclusive prefix sum
  uint32_t stage[65];        // boundary words of the symbols
  uint32_t hstage[68];       // 40 carried bits + 74 + 6 * 316 header bits
};

struct DeflWin { // lane-uniform: what defl_wave_code found
  uint32_t dyn, bits, hbits, hlit, hdist;
};

struct DeflCount {
  uint32_t* f;
  uint32_t nll, nd;
  DMF void lit(uint32_t b) {
    DW_ADD(&f[b], 1u);
    nll++;
  }
  DMF void match(uint32_t l, uint32_t d) {
    uint32_t eb, ev;
    DW_ADD(&f[defl_len_sym(l, &eb, &ev)], 1u);
    DW_ADD(&f[kDeflD0 + defl_dist_sym(d, &eb, &ev)], 1u);
    nll++;
    nd++;
  }
};
struct DeflMeasure {
  const uint8_t* len;
  uint32_t bits;
  DMF void lit(uint32_t b) { bits += len[b]; }
  DMF void match(uint32_t l, uint32_t d) {
    uint32_t eb, ev;
    bits += len[defl_len_sym(l, &eb, &ev)] + eb;
    bits += len[kDeflD0 + defl_dist_sym(d, &eb, &ev)] + eb;
  }
};
// A lane's bit writer.  Words wf (where the lane starts) and we (where the
// next lane starts) are boundary words with the stage slots cf and ce; every
// word between them is the lane's alone.
struct DeflEmit {
  const uint8_t* len;
  const uint16_t* code;
  uint32_t* stage;
  uint8_t* out;
  uint32_t wf, we, cf, ce, w, cnt;
  uint64_t acc;
  DMF void word(uint32_t v) {
    if (w == wf) DW_OR(&stage[cf], v);
    else if (w == we) DW_OR(&stage[ce], v);
    else store32(out + 4 * (size_t)w, v);
    w++;
  }
  DMF void put(uint32_t v, uint32_t nb) { // nb <= 28, cnt < 32
    acc |= (uint64_t)v << cnt;
    cnt += nb;
    if (cnt >= 32) {
      word((uint32_t)acc);
      acc >>= 32;
      cnt -= 32;
    }
  }
  DMF void sym(uint32_t s, uint32_t eb, uint32_t ev) {
    put(code[s] | ev << len[s], len[s] + eb);
  }
  DMF void lit(uint32_t b) { sym(b, 0, 0); }
  DMF void match(uint32_t l, uint32_t d) {
    uint32_t eb, ev, s = defl_len_sym(l, &eb, &ev);
    sym(s, eb, ev);
    s = kDeflD0 + defl_dist_sym(d, &eb, &ev);
    sym(s, eb, ev);
  }
  DMF void finish() {
    if (cnt) word((uint32_t)acc);
  }
};

DFN void dw_seg(uint32_t base, uint32_t wend, uint32_t lane, uint32_t* s0,
                uint32_t* s1) {
  uint32_t seg = (uint32_t)snap_segment_size(wend - base);
  *s0 = wend - base > lane * seg ? base + lane * seg : wend;
  *s1 = wend - *s0 > seg ? *s0 + seg : wend;
}
// `nb` <= 32 bits at bit `at` of a staging area
DFN void dw_stage_put(uint32_t* stage, uint32_t at, uint32_t v, uint32_t nb) {
  (void)nb;
  uint64_t x = (uint64_t)v << (at & 31);
  DW_OR(&stage[at >> 5], (uint32_t)x);
  if (x >> 32) DW_OR(&stage[(at >> 5) + 1], (uint32_t)(x >> 32));
}

// Table, counts, lengths and both forms' sizes of the window [base, wend).
DFN DeflWin defl_wave_code(DeflLds& L, const uint8_t* __restrict__ in,
                           uint32_t base, uint32_t wend, uint32_t zlane) {
  (void)zlane;
  DW_SYNC(); // the walks of the window before are done with the table
  DW_LANES {
    for (uint32_t t = lane; t < (1u << kSnapHashBits); t += 64) L.tab[t] = 0xffffu;
    for (uint32_t i = lane; i < kDeflSyms; i += 64) L.f[i] = 0;
    (&L.cnt[0][0][0])[lane] = 0;
    if (lane < 2) L.tot[lane] = L.top[lane] = L.sum[lane] = 0;
  }
  DW_SYNC();
  DW_LANES {
    for (uint32_t p = base + lane; p + 4 <= wend; p += 64)
      dw_min16(L.tab, (load32(in + p) * kSnapHashMul) >> (32 - kSnapHashBits),
               p - base); // p - base <= 16380 < the 0xffff of an empty slot
  }
  DW_SYNC();
  DW_LANES {
    uint32_t s0, s1;
    dw_seg(base, wend, lane, &s0, &s1);
    DeflCount c = {L.f, 0, 0};
    if (s0 < wend) defl_walk(in, base, s0, s1, L.tab, c);
    if (lane == 63) {
      DW_ADD(&L.f[256], 1u);
      c.nll++;
    }
    if (c.nll) DW_ADD(&L.tot[0], c.nll);
    if (c.nd) DW_ADD(&L.tot[1], c.nd);
  }
  DW_SYNC();
  DW_LANES {
    for (uint32_t i = lane; i < kDeflSyms; i += 64) {
      uint32_t a = i >= kDeflD0, lo = a ? kDeflD0 : 0, fi = L.f[i];
      uint32_t len = 0, rank = 0;
      if (fi) {
        uint32_t total = L.tot[a];
        for (len = 1; (fi << len) < total;) len++;
        for (uint32_t j = lo; j < (a ? kDeflSyms : kDeflD0); j++) {
          uint32_t fj = L.f[j];
          rank += (fj > fi || (fj == fi && j < i)) ? 1u : 0u;
        }
        DW_ADD(&L.cnt[0][a][len], 1u);
        DW_MAX(&L.top[a], i - lo + 1);
      }
      L.len[i] = (uint8_t)len;
      L.rank[i] = (uint16_t)rank;
    }
  }
  DW_SYNC();
  for (uint32_t cur = 0;; cur ^= 1) { // the passes of the length rule
    uint32_t slack0 = 0, slack1 = 0;
    for (uint32_t a = 0; a < 2; a++) {
      uint32_t kraft = 0, used = 0;
      for (uint32_t l = 1; l < 16; l++) {
        kraft += L.cnt[cur][a][l] << (15 - l);
        used += L.cnt[cur][a][l];
      }
      uint32_t slack = used >= 2 ? (1u << 15) - kraft : 0;
      if (a) slack1 = slack;
      else slack0 = slack;
    }
    if (slack0 == 0 && slack1 == 0) break;
    DW_LANES {
      for (uint32_t i = lane; i < kDeflSyms; i += 64) {
        uint32_t len = L.len[i], a = i >= kDeflD0;
        if (len == 0) continue;
        uint32_t slack = a ? slack1 : slack0, start = 0, taken = 0;
        for (uint32_t l = 1; l <= len; l++) {
          uint32_t c = L.cnt[cur][a][l], room = slack >> (15 - l);
          uint32_t t = l == 1 ? 0 : (c < room ? c : room);
          slack -= t << (15 - l);
          if (l == len) taken = t;
          else start += c;
        }
        if (L.rank[i] - start < taken) L.len[i] = (uint8_t)--len;
        DW_ADD(&L.cnt[cur ^ 1][a][len], 1u);
      }
    }
    DW_SYNC();
    DW_LANES {
      if (lane < 32) (&L.cnt[cur][0][0])[lane] = 0;
    }
    DW_SYNC();
  }
  DeflWin win;
  win.hlit = L.top[0] < 257 ? 257 : L.top[0];
  win.hdist = L.top[1] < 1 ? 1 : L.top[1];
  DW_LANES {
    uint32_t dyn = 0, fix = 0, hc = 0;
    for (uint32_t i = lane; i < kDeflSyms; i += 64) {
      uint32_t fi = L.f[i], ex = defl_extra(i);
      dyn += fi * (L.len[i] + ex);
      fix += fi * (defl_fixed_len(i) + ex);
    }
    for (uint32_t i = lane * 5; i < lane * 5 + 5 && i < win.hlit + win.hdist; i++) {
      DeflTok t = defl_hdr_token(L.len, win.hlit, win.hlit + win.hdist, i);
      if (t.sym < 19) hc += defl_cl_len(t.sym) + t.eb;
    }
    L.hcost[lane] = hc;
    DW_ADD(&L.sum[0], dyn + hc);
    DW_ADD(&L.sum[1], fix);
  }
  DW_SYNC();
  uint32_t dynbits = 3 + 14 + 57 + L.sum[0], fixbits = 3 + L.sum[1];
  win.dyn = dynbits < fixbits;
  win.bits = win.dyn ? dynbits : fixbits;
  win.hbits = 3;
  if (win.dyn) {
    win.hbits = 3 + 14 + 57;
    for (uint32_t j = 0; j < 64; j++) win.hbits += L.hcost[j];
  }
  return win;
}

// Writes the window whose code defl_wave_code left in L.  `pos` is the bit of
// the slot at which the window starts, `hb` the output word that hstage[0]
// stands for, carry0/carry1 the bits of the words hb and hb + 1 that are
// already decided; all three move past the window.
DFN void defl_wave_emit(DeflLds& L, const uint8_t* __restrict__ in, uint32_t base,
                        uint32_t wend, const DeflWin& win, uint32_t final,
                        uint8_t* out, uint64_t& pos, uint32_t& hb,
                        uint32_t& carry0, uint32_t& carry1, uint32_t zlane) {
  (void)zlane;
  DW_LANES {
    if (!win.dyn)
      for (uint32_t i = lane; i < kDeflSyms; i += 64)
        L.len[i] = (uint8_t)(i < kDeflD0 + 30 ? defl_fixed_len(i) : 0);
    for (uint32_t i = lane; i < 68; i += 64) L.hstage[i] = 0;
    L.stage[lane] = 0;
    if (lane == 0) L.stage[64] = 0;
  }
  DW_SYNC();
  DW_LANES {
    if (lane < 30) { // lane q - 1 numbers the codes of length q, by symbol
      uint32_t a = lane >= 15, q = lane - 15 * a + 1;
      uint32_t lo = a ? kDeflD0 : 0, hi = a ? kDeflSyms : kDeflD0, next = 0;
      for (uint32_t j = lo; j < hi; j++) {
        uint32_t l = L.len[j];
        if (l && l < q) next += 1u << (q - l);
      }
      for (uint32_t j = lo; j < hi; j++)
        if (L.len[j] == q) L.code[j] = (uint16_t)defl_rev(next++, q);
    }
  }
  DW_SYNC();
  DW_LANES {
    uint32_t s0, s1;
    dw_seg(base, wend, lane, &s0, &s1);
    DeflMeasure m = {L.len, 0};
    if (s0 < wend) defl_walk(in, base, s0, s1, L.tab, m);
    if (lane == 63) m.bits += L.len[256];
    L.lraw[lane] = m.bits;
  }
  DW_SYNC();
  const uint32_t hrel = (uint32_t)(pos - 32 * (uint64_t)hb); // <= 40
  DW_LANES {
    uint32_t o = 0;
    for (uint32_t j = 0; j < lane; j++) o += L.lraw[j];
    L.lbits[lane] = o;
    if (lane == 63) L.lbits[64] = o + L.lraw[63];
    // the header
    if (lane == 0) {
      DW_OR(&L.hstage[0], carry0);
      DW_OR(&L.hstage[1], carry1);
      dw_stage_put(L.hstage, hrel, final | (win.dyn ? 2u : 1u) << 1, 3);
      if (win.dyn)
        dw_stage_put(L.hstage, hrel + 3,
                     (win.hlit - 257) | (win.hdist - 1) << 5 | 15u << 10, 14);
    }
    if (win.dyn) {
      if (lane < 19)
        dw_stage_put(L.hstage, hrel + 17 + 3 * lane,
                     defl_cl_len(defl_cl_order(lane)), 3);
      uint32_t at = hrel + 74, tot = win.hlit + win.hdist;
      for (uint32_t j = 0; j < lane; j++) at += L.hcost[j];
      for (uint32_t i = lane * 5; i < lane * 5 + 5 && i < tot; i++) {
        DeflTok t = defl_hdr_token(L.len, win.hlit, tot, i);
        if (t.sym == 19) continue;
        uint32_t cl = defl_cl_len(t.sym);
        dw_stage_put(L.hstage, at, defl_cl_code(t.sym) | t.ev << cl, cl + t.eb);
        at += cl + t.eb;
      }
    }
  }
  DW_SYNC();
  const uint64_t sym0 = pos + win.hbits; // the first symbol's bit
  const uint32_t hfull = (uint32_t)(sym0 >> 5) - hb;
  DW_LANES {
    for (uint32_t k = lane; k < hfull; k += 64)
      store32(out + 4 * (size_t)(hb + k), L.hstage[k]);
    if (lane == 0) L.stage[0] = L.hstage[hfull]; // zero if sym0 is a word's start
  }
  DW_SYNC();
  DW_LANES {
    uint32_t s0, s1;
    dw_seg(base, wend, lane, &s0, &s1);
    uint64_t b = sym0 + L.lbits[lane];
    DeflEmit e;
    e.len = L.len;
    e.code = L.code;
    e.stage = L.stage;
    e.out = out;
    e.wf = (uint32_t)(b >> 5);
    e.we = (uint32_t)((sym0 + L.lbits[lane + 1]) >> 5);
    e.cf = lane;
    while (e.cf > 0 && (uint32_t)((sym0 + L.lbits[e.cf - 1]) >> 5) == e.wf) e.cf--;
    e.ce = e.we == e.wf ? e.cf : lane + 1;
    e.w = e.wf;
    e.cnt = (uint32_t)b & 31;
    e.acc = 0;
    if (s0 < wend) defl_walk(in, base, s0, s1, L.tab, e);
    if (lane == 63) e.sym(256, 0, 0);
    e.finish();
  }
  DW_SYNC();
  const uint64_t end = sym0 + L.lbits[64];
  const uint32_t wlast = (uint32_t)(end >> 5);
  DW_LANES { // a boundary word's first lane stores it, unless bits may follow
    uint32_t w = (uint32_t)((sym0 + L.lbits[lane]) >> 5);
    bool first = lane == 0 || (uint32_t)((sym0 + L.lbits[lane - 1]) >> 5) != w;
    if (first && w != wlast) store32(out + 4 * (size_t)w, L.stage[lane]);
  }
  uint32_t slot = 64;
  while (slot > 0 && (uint32_t)((sym0 + L.lbits[slot - 1]) >> 5) == wlast) slot--;
  carry0 = (end & 31) ? L.stage[slot] : 0;
  carry1 = 0;
  hb = wlast;
  pos = end;
  DW_SYNC();
}

// The stored payload of block in[0, n), 0 < n <= kDeflMaxUnc, into `out`
// (4-byte aligned): measured over all windows first, and written only if the
// ratio rule accepts it (`force`, the check program's: written anyway).
// Returns the payload's size, or 0 with nothing written.  No store reaches a
// byte at or past that size.
DFN uint32_t defl_enc_wave(DeflLds& L, const uint8_t* __restrict__ in, uint32_t n,
                           uint8_t* out, bool force, uint32_t zlane) {
  uint64_t bits = 0;
  DeflWin win = {0, 0, 0, 0, 0};
  for (uint32_t base = 0; base < n; base += kDeflWindow) {
    win = defl_wave_code(L, in, base, n - base > kDeflWindow ? base + kDeflWindow : n,
                         zlane);
    bits += win.bits;
  }
  uint64_t pre = 0; // varint32(n), at most 40 bits
  uint32_t hl = 0;
  for (uint32_t v = n;; v >>= 7, hl++) {
    pre |= (uint64_t)((v & 0x7f) | (v >= 0x80 ? 0x80 : 0)) << (8 * hl);
    if (v < 0x80) break;
  }
  hl++;
  const uint64_t cn = hl + ((bits + 7) >> 3);
  if (!force && cn > (((uint64_t)896 * n) >> 10)) return 0;
  uint64_t pos = 8 * hl;
  uint32_t hb = 0, carry0 = (uint32_t)pre, carry1 = (uint32_t)(pre >> 32);
  for (uint32_t base = 0; base < n; base += kDeflWindow) {
    uint32_t wend = n - base > kDeflWindow ? base + kDeflWindow : n;
    if (n > kDeflWindow) win = defl_wave_code(L, in, base, wend, zlane);
    defl_wave_emit(L, in, base, wend, win, wend == n, out, pos, hb, carry0,
                   carry1, zlane);
  }
  DW_LANES { // the last, partial word byte by byte: cn may end inside it
    if (lane == 0)
      for (uint64_t t = 4 * (uint64_t)hb; t < cn; t++)
        out[t] = (uint8_t)(carry0 >> (8 * (t - 4 * (uint64_t)hb)));
  }
  return (uint32_t)cn;
}
#endif // DCW_DEFLATE_WAVE

} // namespace dcw
