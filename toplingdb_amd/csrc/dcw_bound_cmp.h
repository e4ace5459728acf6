// dcw_bound_cmp.h — raw bytewise order of a boundary user key of any length
// against a job key, and the range-tombstone fragment lookup built on it.
// Plain C++ shared by the dedup kernel (dcw_k_merge.h) and the host check
// program (tools/gk_host): no wave builtins, no LDS types.
#pragma once
#include "dcw_common.h"

namespace dcw {

// Raw bytewise order (Compare(bound, key) of the bytewise comparator) of a
// boundary user key of ANY length against a job key: <0, 0, >0.
// (b0,b1) / (k0,k1) are the zero-padded 16-byte prefix words.  Where they
// differ the first differing byte decides, as in raw order (a pad byte only
// meets a real byte when the shorter key is a prefix of the longer, and 0 is
// the smallest byte).  Where they tie, fast mode (kfull null, ulen <= 16)
// breaks the tie on length; general mode compares the stored bytes first.
// bext holds min(blen, DCW_GKEY_MAX) bytes: a job key is at most
// DCW_GKEY_MAX long, so of a longer boundary only that prefix and "it is
// longer" matter.
//
// Two boundaries that this function cannot tell apart compare the same way
// against every job key, so a list of boundaries sorted in raw order stays
// monotone under it (the binary searches over levels-below files and
// range-tombstone fragments rely on that):
//  - fast mode, both longer than 16 bytes with equal words: a job key has
//    ulen <= 16, so on a word tie both are longer than it and both come out
//    > key; where the words differ, they differ from the key's in the same
//    place.  Against a boundary of <= 16 bytes with the same words the
//    length compare is the raw order (the shorter one is a prefix).
//  - general mode, both longer than DCW_GKEY_MAX with equal first
//    DCW_GKEY_MAX bytes: ulen <= DCW_GKEY_MAX, so either a byte below ulen
//    decides (the same byte for both) or both are longer than the key.
DCW_HD int bound_cmp(uint64_t b0, uint64_t b1, uint32_t blen,
                     const uint8_t* __restrict__ bext, uint64_t k0,
                     uint64_t k1, uint32_t ulen,
                     const uint8_t* __restrict__ kfull) {
  if (b0 != k0) return b0 < k0 ? -1 : 1;
  if (b1 != k1) return b1 < k1 ? -1 : 1;
  if (kfull) {
    uint32_t m = blen < DCW_GKEY_MAX ? blen : DCW_GKEY_MAX;
    if (ulen < m) m = ulen;
    for (uint32_t t = 0; t < m; t++)
      if (bext[t] != kfull[t]) return bext[t] < kfull[t] ? -1 : 1;
  }
  if (blen != ulen) return blen < ulen ? -1 : 1;
  return 0;
}

// Range-tombstone fragments sorted by start key in raw order (SoA: prefix
// words, true length, and in general mode the first DCW_GKEY_MAX start bytes
// at DCW_GKEY_STRIDE; rd_ext null in fast mode).  Returns the number of
// fragments whose start is <= the job key, so the fragment containing the
// key is the one before that index (0: the key lies before every fragment).
DCW_HD uint32_t rd_frag_upper(const uint64_t* __restrict__ rd_k0,
                              const uint64_t* __restrict__ rd_k1,
                              const uint32_t* __restrict__ rd_len,
                              const uint8_t* __restrict__ rd_ext,
                              uint32_t num_rd, uint64_t k0, uint64_t k1,
                              uint32_t ulen,
                              const uint8_t* __restrict__ kfull) {
  uint32_t lo = 0, hi = num_rd;
  while (lo < hi) {
    uint32_t mid = (lo + hi) / 2;
    bool le = bound_cmp(rd_k0[mid], rd_k1[mid], rd_len[mid],
                        kfull ? rd_ext + (uint64_t)mid * DCW_GKEY_STRIDE
                              : nullptr,
                        k0, k1, ulen, kfull) <= 0;
    if (le)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

} // namespace dcw
