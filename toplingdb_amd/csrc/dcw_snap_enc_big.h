// dcw_snap_enc_big.h — the snappy segment encoder for blocks of any size
// (codec spec v4, dcw_common.h): the general measure/emit pair behind
// k_compress_large (dcw_k_emit.h).  Plain C++ shared by that kernel and the
// host check program (tools/enc_big_host): no wave builtins, no LDS types.
//
// What a block above 16 KiB adds to the default kernel's encoder:
//   literals   a segment is ceil(n/64) bytes, so a literal may be longer
//              than 256 bytes: the header is 1 byte for len-1 < 60, else
//              1 + the byte count of len-1 (little-endian, 1..4 bytes)
//   copies     an offset of 65536 or more takes the 4-byte-offset form,
//              5 bytes per chunk; chunking (<= 64 bytes, tail >= 4) is that
//              of snap_emit_copy
//   positions  u32 in the first-occurrence table (sentinel 0xffffffff;
//              callers keep n < 2^31)
// The emitted bytes equal dcw::snap_encode_segment for every input; only
// the data movement differs (word-wise literal copies, ctz match extension).
//
// One walk serves both passes: snapb_walk_segment<false> measures a
// segment's fragment length without a store, snapb_walk_segment<true> writes
// it.  The two are the same code, so a measured length is the emitted one.
#pragma once
#include "dcw_common.h"

namespace dcw {

// header bytes of a literal of len >= 1 bytes
DCW_HD uint32_t snapb_lit_hdr(uint32_t len) {
  uint32_t n = len - 1;
  if (n < 60) return 1;
  return n < (1u << 8) ? 2 : n < (1u << 16) ? 3 : n < (1u << 24) ? 4 : 5;
}
DCW_HD uint32_t snapb_lit_len(uint32_t len) {
  return len == 0 ? 0 : snapb_lit_hdr(len) + len;
}
// length of what snap_emit_copy (dcw_common.h) writes: the same chunking
DCW_HD uint32_t snapb_copy_len(uint32_t offset, uint32_t len) {
  const uint32_t per = offset < 65536 ? 3 : 5;
  uint32_t c = 0;
  while (len > 0) {
    if (len >= 4 && len <= 11 && offset < 2048) return c + 2;
    uint32_t chunk = len > 64 ? 64 : len;
    if (len - chunk > 0 && len - chunk < 4) chunk = len - 4;
    c += per;
    len -= chunk;
  }
  return c;
}

DCW_HD uint8_t* snapb_emit_literal(uint8_t* op, const uint8_t* lit,
                                   uint32_t len) {
  if (len == 0) return op;
  uint32_t n = len - 1;
  if (n < 60) {
    *op++ = (uint8_t)(n << 2);
  } else {
    uint32_t count = snapb_lit_hdr(len) - 1;
    *op++ = (uint8_t)((59 + count) << 2);
    for (uint32_t i = 0; i < count; i++) *op++ = (uint8_t)(n >> (8 * i));
  }
  uint32_t t = 0;
  for (; t + 4 <= len; t += 4) store32(op + t, load32(lit + t));
  for (; t < len; t++) op[t] = lit[t];
  return op + len;
}

// Walk segment [s0, s1) of in[0, n) against the first-occurrence table tab
// (1 << kSnapHashBits u32 slots, 0xffffffff = empty) and return the length
// of its fragment.  EMIT writes the fragment at op; otherwise op is unused
// and nothing is stored.  Reads stay inside [0, s1): a candidate c lies
// below p, and every load at c + l is matched by one at p + l < s1.
template <bool EMIT>
DCW_HD uint32_t snapb_walk_segment(const uint8_t* __restrict__ in, uint32_t s0,
                                   uint32_t s1,
                                   const uint32_t* __restrict__ tab,
                                   uint8_t* op) {
  uint32_t lit = s0, p = s0, out = 0;
  while (p + 4 <= s1) {
    uint32_t w = load32(in + p);
    uint32_t h = (w * kSnapHashMul) >> (32 - kSnapHashBits);
    uint32_t c = tab[h];
    if (c != 0xffffffffu && c < p && load32(in + c) == w) {
      uint32_t l = 4;
      bool diff = false;
      while (p + l + 4 <= s1) {
        uint32_t x = load32(in + c + l) ^ load32(in + p + l);
        if (x) {
          l += (uint32_t)__builtin_ctz(x) >> 3;
          diff = true;
          break;
        }
        l += 4;
      }
      if (!diff)
        while (p + l < s1 && in[c + l] == in[p + l]) l++;
      out += snapb_lit_len(p - lit) + snapb_copy_len(p - c, l);
      if (EMIT) {
        op = snapb_emit_literal(op, in + lit, p - lit);
        op = snap_emit_copy(op, p - c, l);
      }
      p += l;
      lit = p;
    } else {
      p++;
    }
  }
  out += snapb_lit_len(s1 - lit);
  if (EMIT) (void)snapb_emit_literal(op, in + lit, s1 - lit);
  return out;
}

} // namespace dcw
