// dcw_snap_dec_lds.h — the serial snappy decoder for LDS-staged blocks.
// Included by dcw_k_decode.h for the GPU and, with __device__ and
// __forceinline__ defined away, by the host fuzz harnesses under
// tools/dec_host_fuzz.  Plain C++ only: no wave builtins, no LDS types.
#pragma once
#include <cstdint>
#include <cstring>

namespace dcw {

// two unaligned 32-bit DS ops: unaligned ds_read/write_b32 is penalty-free
// on CDNA4, while an align(1) 8-byte memcpy is lowered to EIGHT ds_*_u8
// (and an unaligned _b64 would replay at 64 cycles) — this is the decoder's
// dominant instruction, so the width matters more than anything else in it
__device__ __forceinline__ uint64_t lds_ld64(const uint8_t* p) {
  uint32_t lo, hi;
  memcpy(&lo, p, 4);
  memcpy(&hi, p + 4, 4);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
__device__ __forceinline__ void lds_st64(uint8_t* p, uint64_t v) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  memcpy(p, &lo, 4);
  memcpy(p + 4, &hi, 4);
}
// Serial snappy decoder specialized for LDS-staged blocks.  The generic
// DCW_HD decoder compiles to a dependent ds_read -> waitcnt -> ds_write
// chain PER WORD (and 2-3 chained byte reads per tag), which is what made
// k_decompress ~30% of all kernel time.  Here each op does ONE unaligned
// 8-byte header fetch (tag + length/offset bytes decoded from registers),
// literals move 16 B per round trip, and short-offset overlapped copies
// use pattern doubling.  Stores may run up to 15 B past the logical
// output end and header fetches up to 7 B past the input end: both stay
// inside DEC_PAD, and every ACCEPT decision is bounds-checked against the
// true n/ulen first, so accepted output bytes are identical to the
// generic decoder's and corrupt blocks are rejected the same way.
template <int PIPE>
__device__ uint32_t snap_dec_lds(const uint8_t* __restrict__ in, uint32_t n,
                                 uint8_t* __restrict__ out, uint32_t cap) {
  uint32_t ulen = 0, ip = 0;
  {
    uint64_t h = lds_ld64(in);
    uint32_t s = 0;
    for (;;) {
      if (ip >= n || ip >= 5) return 0;
      uint8_t b = (uint8_t)(h >> (8 * ip));
      ulen |= (uint32_t)(b & 0x7f) << s;
      ip++;
      if (!(b & 0x80)) break;
      s += 7;
    }
  }
  if (ulen > cap) return 0;
  uint32_t op = 0;
  // PIPE=1 software-pipelines the header: the next op's position is known
  // before the current op's copy runs, so its 8-byte fetch is issued ahead
  // of the copy and the LDS round trip overlaps the data movement
  uint64_t h = lds_ld64(in + ip);
  while (ip < n) {
    if (!PIPE) h = lds_ld64(in + ip);
    uint8_t tag = (uint8_t)h;
    if ((tag & 3) == 0) { // literal
      uint32_t len = (uint32_t)(tag >> 2) + 1;
      uint32_t hb = 1;
      if (len > 60) {
        uint32_t nb = len - 60; // 1..4 length bytes, little-endian
        if (ip + 1 + nb > n) return 0;
        uint32_t lm1 = (uint32_t)((h >> 8) & (0xffffffffull >> (8 * (4 - nb))));
        // a 4-byte length near 2^32 would wrap len / ip + len below
        if (lm1 >= n) return 0;
        len = lm1 + 1;
        hb = 1 + nb;
      }
      ip += hb;
      if (ip + len > n || op + len > ulen) return 0;
      uint64_t hn = PIPE ? lds_ld64(in + ip + len) : 0;
      for (uint32_t i = 0; i < len; i += 16) {
        uint64_t a = lds_ld64(in + ip + i);
        uint64_t b = lds_ld64(in + ip + i + 8);
        lds_st64(out + op + i, a);
        lds_st64(out + op + i + 8, b);
      }
      ip += len;
      op += len;
      if (PIPE) h = hn;
    } else { // copy
      uint32_t len, offset, hb;
      if ((tag & 3) == 1) {
        len = ((uint32_t)(tag >> 2) & 7) + 4;
        offset = ((uint32_t)(tag >> 5) << 8) | (uint8_t)(h >> 8);
        hb = 2;
      } else if ((tag & 3) == 2) {
        len = (uint32_t)(tag >> 2) + 1;
        offset = (uint32_t)(h >> 8) & 0xffffu;
        hb = 3;
      } else {
        len = (uint32_t)(tag >> 2) + 1;
        offset = (uint32_t)(h >> 8);
        hb = 5;
      }
      if (ip + hb > n) return 0;
      ip += hb;
      if (offset == 0 || offset > op || op + len > ulen) return 0;
      uint64_t hn = PIPE ? lds_ld64(in + ip) : 0;
      uint32_t src = op - offset;
      uint32_t end = op + len;
      if (offset >= 16) {
        for (uint32_t i = 0; i < len; i += 16) {
          uint64_t a = lds_ld64(out + src + i);
          uint64_t b = lds_ld64(out + src + i + 8);
          lds_st64(out + op + i, a);
          lds_st64(out + op + i + 8, b);
        }
      } else if (offset >= 8) {
        for (uint32_t i = 0; i < len; i += 8)
          lds_st64(out + op + i, lds_ld64(out + src + i));
      } else {
        // pattern doubling: each 8-B store validates (op-src) more bytes
        // and the usable distance doubles; reads of not-yet-valid bytes
        // land beyond the advancing point and are overwritten next round
        while (op < end) {
          lds_st64(out + op, lds_ld64(out + src));
          uint32_t d = op - src;
          if (d >= 8) {
            for (uint32_t i = 8; op + i < end; i += 8)
              lds_st64(out + op + i, lds_ld64(out + src + i));
            break;
          }
          op += d < end - op ? d : end - op;
        }
      }
      op = end;
      if (PIPE) h = hn;
    }
  }
  return op == ulen ? ulen : 0;
}

} // namespace dcw
