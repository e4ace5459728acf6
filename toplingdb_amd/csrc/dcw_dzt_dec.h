// dcw_dzt_dec.h — decode side of DcwZipTable ("DZT1") inputs: the
// dict-snappy value-block decoder and the key-block record decoder.
// Plain C++ shared by the device kernels (dcw_k_dzt_in.h) and the host
// check program (tools/dzt_in_host): no wave builtins, no LDS types.
// Format: oracle/dzt.c header comment; codec: "DZT dict codec v1"
// (dcw_common.h, snappy_uncompress_dict is the reference restatement).
#pragma once
#include "dcw_common.h"

namespace dcw {

enum DztDecErr : int {
  DZT_OK = 0,
  DZT_E_SNAPPY = 2,      // == DE_SNAPPY
  DZT_E_BLOCK_PARSE = 3, // == DE_BLOCK_PARSE
  DZT_E_UKEY_LEN = 4,    // == DE_UKEY_LEN
  DZT_E_TYPE = 5,        // == DE_TYPE
};

static const uint32_t kDztKeysPerBlock = 64;
static const uint32_t kDztUkeyMax = 48; // general-key envelope (DCW_GKEY_MAX)

// Decode one dict-snappy stream in[0,n) into out[0,cap), against the
// dictionary dict[0,D).  Accepts exactly the streams snappy_uncompress_dict
// accepts: literals with 0..4 length bytes, the 1-, 2- and 4-byte-offset
// copy forms, copies sourced from the dict, copies that start in the dict
// and run on into the block, in-block copies and overlapping ones.  Every
// length is compared against the bytes that remain (n - ip, ulen - op)
// BEFORE it is added to a position, so no sum can wrap: a 4-byte literal
// length near 2^32 is refused while it is still a bare number.  Writes
// never pass out + ulen and reads never pass in + n or dict + D.
// Returns 0 and *ulen_out on success, DZT_E_SNAPPY on any corruption.
DCW_HD int dzt_snap_dec(const uint8_t* __restrict__ dict, uint32_t D,
                        const uint8_t* __restrict__ in, uint32_t n,
                        uint8_t* __restrict__ out, uint32_t cap,
                        uint32_t* ulen_out) {
  uint32_t ulen = 0, ip = 0;
  for (uint32_t s = 0;; s += 7) {
    if (ip >= n || s > 28) return DZT_E_SNAPPY;
    uint8_t b = in[ip++];
    ulen |= (uint32_t)(b & 0x7f) << s;
    if (!(b & 0x80)) break;
  }
  if (ulen > cap) return DZT_E_SNAPPY;
  uint32_t op = 0;
  while (ip < n) {
    uint8_t tag = in[ip++];
    if ((tag & 3) == 0) { // literal
      uint32_t len = (uint32_t)(tag >> 2) + 1;
      if (len > 60) {
        uint32_t nb = len - 60; // 1..4 length bytes, little-endian
        if (nb > n - ip) return DZT_E_SNAPPY;
        uint32_t lm1 = 0;
        for (uint32_t i = 0; i < nb; i++) lm1 |= (uint32_t)in[ip + i] << (8 * i);
        ip += nb;
        // a literal cannot be longer than the stream that carries it; this
        // also keeps lm1 + 1 from wrapping at 2^32
        if (lm1 >= n) return DZT_E_SNAPPY;
        len = lm1 + 1;
      }
      if (len > n - ip || len > ulen - op) return DZT_E_SNAPPY;
      uint32_t i = 0;
      for (; i + 4 <= len; i += 4) store32(out + op + i, load32(in + ip + i));
      for (; i < len; i++) out[op + i] = in[ip + i];
      ip += len;
      op += len;
    } else { // copy
      uint32_t len, offset;
      if ((tag & 3) == 1) {
        if (n - ip < 1) return DZT_E_SNAPPY;
        len = ((uint32_t)(tag >> 2) & 7) + 4;
        offset = ((uint32_t)(tag >> 5) << 8) | in[ip];
        ip += 1;
      } else if ((tag & 3) == 2) {
        if (n - ip < 2) return DZT_E_SNAPPY;
        len = (uint32_t)(tag >> 2) + 1;
        offset = (uint32_t)in[ip] | ((uint32_t)in[ip + 1] << 8);
        ip += 2;
      } else {
        if (n - ip < 4) return DZT_E_SNAPPY;
        len = (uint32_t)(tag >> 2) + 1;
        offset = load32(in + ip);
        ip += 4;
      }
      // the source must start inside dict || produced: offset in [1, op + D]
      // (compared without forming op + D, so a huge offset cannot wrap)
      if (offset == 0 || (offset > op && offset - op > D) || len > ulen - op)
        return DZT_E_SNAPPY;
      uint32_t i = 0;
      if (offset > op) { // starts in the dict, `back` bytes before its end
        uint32_t back = offset - op;
        uint32_t m = len < back ? len : back;
        const uint8_t* dsrc = dict + (D - back);
        for (; i < m; i++) out[op + i] = dsrc[i];
      }
      // the rest (all of it for an in-block copy) comes from out, at
      // distance `offset`; forward order makes overlapping copies repeat
      // (op + i >= offset from here on, so the index does not go negative)
      if (offset >= 4)
        for (; i + 4 <= len; i += 4)
          store32(out + op + i, load32(out + (op + i - offset)));
      for (; i < len; i++) out[op + i] = out[op + i - offset];
      op += len;
    }
  }
  if (op != ulen) return DZT_E_SNAPPY;
  *ulen_out = ulen;
  return DZT_OK;
}

// One record of a key block (oracle/dzt.c KEY AREA).
struct DztKeyRec {
  uint64_t tag;
  uint32_t voff, vlen;
};

// Decode the record at *pos of the key block kb[0,ksize).  `key` holds the
// previous record's user key (U bytes) and receives this one's; prev_tag is
// the previous record's tag.  first = the block's first record.  Checks, in
// this order: both varints inside the block; shared_u <= U (BLOCK_PARSE);
// shared_u + nonshared_u == U (UKEY_LEN); shared_u == 0 on the first
// record; the whole record inside ksize; value type in {Put, Delete,
// SingleDelete} (TYPE); order against the previous record — user key
// ascending, tag descending on a tie (BLOCK_PARSE).
DCW_HD int dzt_key_next(const uint8_t* __restrict__ kb, uint32_t ksize,
                        uint32_t* pos, uint32_t U, bool first, uint8_t* key,
                        uint64_t prev_tag, DztKeyRec* r) {
  uint32_t p = *pos, sh, ns;
  int m = varint32_get(kb + p, kb + ksize, &sh);
  if (m < 0) return DZT_E_BLOCK_PARSE;
  p += (uint32_t)m;
  m = varint32_get(kb + p, kb + ksize, &ns);
  if (m < 0) return DZT_E_BLOCK_PARSE;
  p += (uint32_t)m;
  if (sh > U) return DZT_E_BLOCK_PARSE;
  if (ns != U - sh) return DZT_E_UKEY_LEN;
  if (first && sh != 0) return DZT_E_BLOCK_PARSE;
  // ns <= U <= 48, so p + ns + 16 cannot wrap
  if (ksize - p < ns + 16) return DZT_E_BLOCK_PARSE;
  int cmp = 0; // this key vs the previous one (they agree on [0, sh))
  for (uint32_t t = 0; t < ns; t++) {
    uint8_t nb = kb[p + t], pb = key[sh + t];
    if (cmp == 0 && nb != pb) cmp = nb > pb ? 1 : -1;
    key[sh + t] = nb;
  }
  p += ns;
  r->tag = load64(kb + p);
  r->voff = load32(kb + p + 8);
  r->vlen = load32(kb + p + 12);
  p += 16;
  uint8_t vt = (uint8_t)r->tag;
  if (!(vt == kTypeValue || vt == kTypeDeletion || vt == kTypeSingleDeletion))
    return DZT_E_TYPE;
  if (!first && (cmp < 0 || (cmp == 0 && r->tag >= prev_tag)))
    return DZT_E_BLOCK_PARSE;
  *pos = p;
  return DZT_OK;
}

} // namespace dcw
