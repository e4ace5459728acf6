// dcw_dzt_enc.h — build side of the DcwZipTable ("DZT1") key area: the
// key-record size rule and the key-record writer.  Plain C++ shared by the
// general-key key-area kernel (dcw_k_filter_dzt.h), the file planner
// (dcw_host.cpp) and the host check program (tools/gk_host): no wave
// builtins, no LDS types.  Format: oracle/dzt.c header comment (KEY AREA).
#pragma once
#include "dcw_common.h"

namespace dcw {

// user-key prefix a record shares with the previous one: the internal-key
// prefix `shared_ikey` can run into the tag when two versions of one user
// key follow each other, so it is clamped to U; a block's first record
// shares nothing
DCW_HD uint32_t dzt_krec_shared(uint32_t shared_ikey, uint32_t U,
                                bool block_first) {
  if (block_first) return 0;
  return shared_ikey < U ? shared_ikey : U;
}

// byte size of the record of a U-byte user key that shares `sh` bytes
DCW_HD uint32_t dzt_krec_size(uint32_t sh, uint32_t U) {
  uint32_t ns = U - sh;
  return (uint32_t)varint_len(sh) + (uint32_t)varint_len(ns) + ns + 8 + 4 + 4;
}

// n <= DCW_GKEY_MAX key bytes in 8- and 4-byte moves with a byte tail.
// Neither side is aligned in general: the loads and stores are
// memcpy-typed, so the compiler picks accesses that are legal unaligned.
DCW_HD void dzt_copy_bytes(uint8_t* __restrict__ dst,
                           const uint8_t* __restrict__ src, uint32_t n) {
  uint32_t t = 0;
  for (; t + 8 <= n; t += 8) store64(dst + t, load64(src + t));
  if (t + 4 <= n) {
    store32(dst + t, load32(src + t));
    t += 4;
  }
  for (; t < n; t++) dst[t] = src[t];
}

// Writes one record at p: varint(sh) varint(U - sh) ukey[sh, U) tag voff
// vlen, and returns its size (== dzt_krec_size(sh, U)).  `ukey` points at
// the full user key (U <= DCW_GKEY_MAX bytes readable); the non-shared
// suffix goes straight from there into the record.
DCW_HD uint32_t dzt_krec_put(uint8_t* __restrict__ p, uint32_t sh, uint32_t U,
                             const uint8_t* __restrict__ ukey, uint64_t tag,
                             uint32_t voff, uint32_t vlen) {
  uint8_t* p0 = p;
  uint32_t ns = U - sh;
  p += varint32_put(p, sh);
  p += varint32_put(p, ns);
  dzt_copy_bytes(p, ukey + sh, ns);
  p += ns;
  store64(p, tag);
  store32(p + 8, voff);
  store32(p + 12, vlen);
  return (uint32_t)(p + 16 - p0);
}

} // namespace dcw
