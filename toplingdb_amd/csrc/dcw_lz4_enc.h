// dcw_lz4_enc.h — the LZ4 block encoder for output data blocks of type 4
// (LZ4) and 5 (LZ4HC): one encoder, the types differ in the trailer byte
// only.  Plain C++ shared by k_compress_lz4 (dcw_k_emit.h), dcw_host.cpp and
// the host check program (tools/lz4_enc_host): no wave builtins, no LDS
// types.  The decoder is dcw_lz4_dec.h.
//
// "DCW LZ4 codec v1" (self-pinned like the snappy codec; any
// LZ4 block decoder reads it).  A stored block is varint32(n) + one raw LZ4
// block, a pure function of the block's bytes in[0, n):
//   windows   [w*65536, min((w+1)*65536, n)); matches are found inside a
//             window only, so offsets are <= 65535 and window-relative
//             positions fit u16 (0xffff = empty slot) at any block size
//   table     per window, 1 << kSnapHashBits slots, the snappy codec's hash;
//             a slot holds the SMALLEST position p of the window, p + 4 <=
//             window end, with that hash (order-independent)
//   segments  per window, seg = snap_segment_size(window length); lane i
//             owns [base + i*seg, min(base + (i+1)*seg, window end))
//   walk      of a segment [s0, s1): p = s0; while p + 4 <= s1 and p + 12 <=
//             n: candidate c = tab[h(p)] matches if c < p and load32(c) ==
//             load32(p); the match is extended while p + l < min(s1, n - 5);
//             p += l, else p += 1.  These are the format's end rules: the
//             last match starts 12 bytes before the end, the last 5 bytes
//             are literals
//   stream    all matches in position order, one sequence each; the bytes
//             between two matches are the literals of the later one, across
//             segment and window borders; the last sequence is literals only
//   accept    stored compressed iff preamble + stream <= (896*n) >> 10
//
// A lane's trailing literals belong to a sequence that a later lane closes,
// so a segment is summarised (Lz4Seg) and the summaries are joined by the
// seam scan (lz4_seam); lz4_lane_bytes and lz4_emit_lane then place and
// write one lane's share.  lz4_encode_block is the serial restatement.
#pragma once
#include "dcw_common.h"

namespace dcw {

static const uint32_t kLz4Window = 65536;
static const uint32_t kLz4MaxUnc = 0x7fffffffu; // 32-bit sums stay exact

DCW_HD size_t lz4_max_compressed(size_t n) { return n + n / 255 + 16; }

// a length field: `x` is the literal length, or the match length - 4; the
// nibble holds min(x, 15), the extension bytes the rest
DCW_HD uint32_t lz4_ext_len(uint32_t x) {
  return x < 15 ? 0 : 1 + (x - 15) / 255;
}
DCW_HD uint8_t* lz4_put_ext(uint8_t* op, uint32_t x) {
  if (x < 15) return op;
  for (x -= 15; x >= 255; x -= 255) *op++ = 255;
  *op++ = (uint8_t)x;
  return op;
}
// token + literal-length extension of a sequence of `ll` literals whose
// match nibble is `nib`
DCW_HD uint8_t* lz4_put_head(uint8_t* op, uint32_t ll, uint32_t nib) {
  *op++ = (uint8_t)(((ll < 15 ? ll : 15) << 4) | nib);
  return lz4_put_ext(op, ll);
}
DCW_HD uint8_t* lz4_copy(uint8_t* op, const uint8_t* src, uint32_t len) {
  uint32_t t = 0;
  for (; t + 4 <= len; t += 4) store32(op + t, load32(src + t));
  for (; t < len; t++) op[t] = src[t];
  return op + len;
}

// Length of the match at p, 0 for none; `lim` = min(s1, n - 5) bounds its
// end.  tab holds window-relative positions.  Reads stay below lim: the
// candidate lies below p, and a load at c + l is paired with one at p + l.
DCW_HD uint32_t lz4_match_at(const uint8_t* __restrict__ in, uint32_t base,
                             uint32_t p, uint32_t lim,
                             const uint16_t* __restrict__ tab, uint32_t* off) {
  uint32_t w = load32(in + p);
  uint32_t c = tab[(w * kSnapHashMul) >> (32 - kSnapHashBits)];
  if (c == 0xffffu) return 0;
  c += base;
  if (c >= p || load32(in + c) != w) return 0;
  *off = p - c;
  uint32_t l = 4;
  while (p + l + 4 <= lim) {
    uint32_t x = load32(in + c + l) ^ load32(in + p + l);
    if (x) return l + ((uint32_t)__builtin_ctz(x) >> 3);
    l += 4;
  }
  while (p + l < lim && in[c + l] == in[p + l]) l++;
  return l;
}

// One segment's summary.  With a match: `lead` literals before the first
// match (they end the sequence some earlier lane began), `nib` that match's
// nibble, `body` the bytes from its offset field through the last match's
// end (whole sequences after the first), `trail` literals after the last
// match.  Without one: trail is the whole segment.
struct Lz4Seg {
  uint32_t has, lead, nib, body, trail;
};

// Walk segment [s0, s1) of the window at `base`.  EMIT writes lead + body
// bytes at op (the lead literals, then the body); otherwise op is unused and
// nothing is stored.  The two are the same code, so a measured length is the
// emitted one.
template <bool EMIT>
DCW_HD Lz4Seg lz4_walk_segment(const uint8_t* __restrict__ in, uint32_t n,
                               uint32_t base, uint32_t s0, uint32_t s1,
                               const uint16_t* __restrict__ tab, uint8_t* op) {
  Lz4Seg r = {0, 0, 0, 0, 0};
  uint32_t lit = s0, p = s0;
  const uint32_t lim = n < 5 ? 0 : (s1 < n - 5 ? s1 : n - 5);
  while (p + 4 <= s1 && p + 12 <= n) {
    uint32_t off = 0;
    uint32_t l = lz4_match_at(in, base, p, lim, tab, &off);
    if (l == 0) {
      p++;
      continue;
    }
    uint32_t ll = p - lit, m = l - 4;
    if (!r.has) {
      r.has = 1;
      r.lead = ll;
      r.nib = m < 15 ? m : 15;
    } else {
      r.body += 1 + lz4_ext_len(ll) + ll;
      if (EMIT) op = lz4_put_head(op, ll, m < 15 ? m : 15);
    }
    r.body += 2 + lz4_ext_len(m);
    if (EMIT) {
      op = lz4_copy(op, in + lit, ll);
      *op++ = (uint8_t)off;
      *op++ = (uint8_t)(off >> 8);
      op = lz4_put_ext(op, m);
    }
    p += l;
    lit = p;
  }
  r.trail = s1 - lit;
  return r;
}

// The seam scan's element: the literals that run up to a lane's end, and
// whether a match cut them off from the lanes before.  lz4_seam is
// associative: writing (h, t) for an element, (a ∘ b) ∘ c and a ∘ (b ∘ c)
// are both c if c.h; else (1, b.t + c.t) if b.h; else (a.h, a.t + b.t +
// c.t).  An exclusive scan so gives each lane the literal count carried
// into it from the lanes before (its window's carry-in added where no lane
// before has a match).
struct Lz4Carry {
  uint32_t has, trail;
};
DCW_HD Lz4Carry lz4_seam(Lz4Carry a, Lz4Carry b) {
  Lz4Carry r = {b.has ? 1u : a.has, b.has ? b.trail : a.trail + b.trail};
  return r;
}

// A lane's share of its window's bytes, in stream order: lead, body, then,
// if a later lane of the window has a match (`later`), the head of the
// sequence that lane closes (`lnext` literals) and this lane's trail.
// Literals behind the window's last match are not placed here: they are the
// window's carry-out.
DCW_HD uint32_t lz4_lane_bytes(const Lz4Seg& r, uint32_t later, uint32_t lnext) {
  uint32_t b = r.has ? r.lead + r.body : 0;
  if (later) b += r.trail + (r.has ? 1 + lz4_ext_len(lnext) : 0);
  return b;
}
// Writes exactly lz4_lane_bytes(...) bytes at op; `r` is the measured
// summary of the same segment.
DCW_HD void lz4_emit_lane(const uint8_t* __restrict__ in, uint32_t n,
                          uint32_t base, uint32_t s0, uint32_t s1,
                          const uint16_t* __restrict__ tab, const Lz4Seg& r,
                          uint32_t later, uint32_t lnext, uint32_t nibnext,
                          uint8_t* op) {
  if (r.has) {
    (void)lz4_walk_segment<true>(in, n, base, s0, s1, tab, op);
    op += r.lead + r.body;
    if (later) op = lz4_put_head(op, lnext, nibnext);
  }
  if (later) (void)lz4_copy(op, in + (s1 - r.trail), r.trail);
}

// Serial restatement: windows and segments in order, one running literal
// anchor.  Writes varint32(n) + the stream, at most 5 + lz4_max_compressed(n)
// bytes, and returns their count.  n <= kLz4MaxUnc.
DCW_HD size_t lz4_encode_block(const uint8_t* in, uint32_t n, uint8_t* out) {
  uint8_t* op = out + varint32_put(out, n);
  uint16_t tab[1u << kSnapHashBits];
  uint32_t lit = 0;
  for (uint32_t base = 0; base < n; base += kLz4Window) {
    uint32_t wend = n - base > kLz4Window ? base + kLz4Window : n;
    for (uint32_t t = 0; t < (1u << kSnapHashBits); t++) tab[t] = 0xffffu;
    for (uint32_t p = base; p + 4 <= wend; p++) {
      uint32_t h = (load32(in + p) * kSnapHashMul) >> (32 - kSnapHashBits);
      if (tab[h] == 0xffffu) tab[h] = (uint16_t)(p - base);
    }
    uint32_t seg = (uint32_t)snap_segment_size(wend - base);
    for (uint32_t s0 = base; s0 < wend; s0 += seg) {
      uint32_t s1 = wend - s0 > seg ? s0 + seg : wend;
      uint32_t lim = s1 < n - 5 ? s1 : n - 5; // used only where n >= 12
      for (uint32_t p = s0; p + 4 <= s1 && p + 12 <= n;) {
        uint32_t off = 0;
        uint32_t l = lz4_match_at(in, base, p, lim, tab, &off);
        if (l == 0) {
          p++;
          continue;
        }
        uint32_t m = l - 4;
        op = lz4_put_head(op, p - lit, m < 15 ? m : 15);
        op = lz4_copy(op, in + lit, p - lit);
        *op++ = (uint8_t)off;
        *op++ = (uint8_t)(off >> 8);
        op = lz4_put_ext(op, m);
        p += l;
        lit = p;
      }
    }
  }
  op = lz4_put_head(op, n - lit, 0);
  op = lz4_copy(op, in + lit, n - lit);
  return (size_t)(op - out);
}

} // namespace dcw
