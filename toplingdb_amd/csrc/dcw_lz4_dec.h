// dcw_lz4_dec.h — LZ4 block decoders for input data blocks of type 4 (LZ4)
// and 5 (LZ4HC): the two types decode identically.  Included by
// dcw_k_decode.h for the GPU and by dcw_host.cpp and tools/lz4_host for the
// host (lz4_dec and lz4_preamble; lz4_dec_lds is device code that the host
// tool asks for with DCW_LZ4_LDS_ON_HOST, __device__ and __forceinline__
// defined away as tools/dec_host_fuzz does for snap_dec_lds).  Plain C++
// only: no wave builtins, no LDS types.
//
// A stored block is varint32(uncompressed size) + one raw LZ4 block; the
// functions below take the raw block (`in`, `n`) and the promised size
// (`cap`).  A raw block is a run of sequences: token (high nibble literal
// length, low nibble match length - 4; a nibble of 15 is extended by bytes
// that each add 0..255, the first below 255 ending it), the literals, a
// 2-byte little-endian offset, the match-length extension.  The last
// sequence ends after its literals.
//
// Acceptance rule (tests/foreign_lz4.py states it in Python): loop while
// input remains; read token and literal length, copy the literals; if the
// input is now exhausted the block ends; otherwise read offset and match
// length and copy the match.  Accepted iff the input is consumed exactly
// and exactly `cap` bytes were produced.  liblz4's end-of-block rules (last
// 5 bytes literal, last match 12 bytes before the end) bind encoders only
// and are not enforced: the decoding of a stream is unique either way.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#include <hip/hip_runtime.h>
#define DCW_LZ4_FN __host__ __device__ inline
#define DCW_LZ4_FN_M __host__ __device__
#define DCW_LZ4_LDS 1
#else
#define DCW_LZ4_FN static inline
#define DCW_LZ4_FN_M
#ifdef DCW_LZ4_LDS_ON_HOST
#define DCW_LZ4_LDS 1
#endif
#endif
#ifdef DCW_LZ4_LDS
#include "dcw_snap_dec_lds.h" // lds_ld64 / lds_st64
#endif

namespace dcw {

// varint32 preamble of a stored type-4/5 block: bytes consumed, or -1 for
// a preamble that is cut short or still continues after 5 bytes
DCW_LZ4_FN int lz4_preamble(const uint8_t* p, uint32_t n, uint32_t* usize) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < n && i < 5; i++) {
    r |= (uint32_t)(p[i] & 0x7f) << (7 * i);
    if (!(p[i] & 0x80)) {
      *usize = r;
      return (int)i + 1;
    }
  }
  return -1;
}

// A preset dictionary (util/compression.h:1189-1196: LZ4_setStreamDecode with
// the file's "rocksdb.compression_dict" block, then
// LZ4_decompress_safe_continue): its bytes count as output produced before the
// block's first byte, so an offset may reach back into the dictionary's tail.
// Offsets have 16 bits: only the last 65535 bytes can be reached.  Both
// decoders below take the dictionary as a last argument; Lz4NoDict, the
// default, folds away and leaves them what they are without one.
struct Lz4NoDict {
  static constexpr uint32_t len() { return 0; }
  static constexpr const uint8_t* end() { return nullptr; }
};
struct Lz4Dict {
  const uint8_t* e; // one past the dictionary's last byte
  uint32_t n;       // min(size, 65535)
  DCW_LZ4_FN_M uint32_t len() const { return n; }
  DCW_LZ4_FN_M const uint8_t* end() const { return e; }
};
// The part of a match at out[op] that lies in the dictionary (offset > op;
// offset <= op + len was checked): bytes moved.  What is left is the usual
// move at the same offset, whose source is then out[0].
template <class D>
DCW_LZ4_FN uint32_t lz4_dict_part(const D& dict, uint8_t* out, uint32_t op,
                                  uint32_t offset, uint32_t ml) {
  const uint32_t need = offset - op, c = need < ml ? need : ml;
  const uint8_t* s = dict.end() - need;
  for (uint32_t i = 0; i < c; i++) out[op + i] = s[i];
  return c;
}

#ifdef DCW_LZ4_LDS
// Length extension out of the register window.  `h` holds the 8 bytes at
// `hb`; `ip` (hb <= ip <= hb + 8) is the next byte to consume.  Each round
// takes every byte the window still holds — 7 behind a token, 6 behind an
// offset, 8 after a refetch — with one compare and one count-trailing-
// zeros: no byte loop over LDS.  `room` is what the length may not exceed
// (input left, for literals; output left, for matches): the walk refuses
// as soon as it does, so the 32-bit sum cannot wrap.  Window bytes at or
// past `n` are slack; no decision is taken on them: a terminator found
// there means the real bytes were all 255, an unterminated extension.
__device__ __forceinline__ bool lz4_ext_win(const uint8_t* in, uint32_t n,
                                             uint64_t& h, uint32_t& hb,
                                             uint32_t& ip, uint32_t& len,
                                             uint32_t room) {
  for (;;) {
    uint32_t avail = hb + 8 - ip;
    if (avail == 0) {
      if (ip >= n) return false;
      h = lds_ld64(in + ip);
      hb = ip;
      avail = 8;
    }
    uint64_t w = h >> (8 * (ip - hb));
    uint64_t mask = avail == 8 ? ~0ull : (1ull << (8 * avail)) - 1;
    uint64_t x = ~w & mask; // a non-zero byte of x: that byte is below 255
    if (x == 0) {
      if (ip + avail > n) return false;
      len += 255 * avail;
      ip += avail;
      if (len > room) return false;
      continue;
    }
    uint32_t k = (uint32_t)__builtin_ctzll(x) >> 3;
    if (ip + k >= n) return false;
    len += 255 * k + (uint32_t)(uint8_t)(w >> (8 * k));
    ip += k + 1;
    return len <= room;
  }
}

// Serial decoder for LDS-staged blocks (n, cap <= DEC_MAX; both buffers
// carry DEC_PAD bytes of slack).  One unaligned 8-byte fetch at the token:
// with a literal length of 5 or less and no extension — the common case in
// prefix-coded key/value blocks — that window also holds the offset, and
// the whole sequence costs one header fetch; otherwise the offset takes a
// second fetch, issued before the literals move.  Literals move 16 B per
// round trip; matches move 16 B at a time from offset 16 up, 8 B at a time
// for offsets 8..15, and by pattern doubling below that.  Stores may run
// up to 15 B past the output end, literal loads up to 15 B and header
// fetches up to 7 B past the input end: all inside DEC_PAD.  Every accept
// or refuse decision is taken against the true n and cap before the move.
template <class D = Lz4NoDict>
__device__ inline bool lz4_dec_lds(const uint8_t* __restrict__ in, uint32_t n,
                            uint8_t* __restrict__ out, uint32_t cap,
                            const D& dict = D()) {
  uint32_t ip = 0, op = 0;
  while (ip < n) {
    uint64_t h = lds_ld64(in + ip);
    uint32_t hb = ip;
    uint32_t tok = (uint8_t)h;
    uint32_t ll = tok >> 4, ml = (tok & 15) + 4;
    ip++;
    if (ll == 15 && !lz4_ext_win(in, n, h, hb, ip, ll, n - ip)) return false;
    if (ll > n - ip || ll > cap - op) return false;
    uint32_t at = ip + ll; // the offset's position, or n at the block's end
    bool in_win = at + 2 <= hb + 8;
    uint64_t h2 = 0;
    if (!in_win && at < n) h2 = lds_ld64(in + at);
    for (uint32_t i = 0; i < ll; i += 16) {
      uint64_t a = lds_ld64(in + ip + i);
      uint64_t b = lds_ld64(in + ip + i + 8);
      lds_st64(out + op + i, a);
      lds_st64(out + op + i + 8, b);
    }
    ip = at;
    op += ll;
    if (ip == n) break;
    if (ip + 2 > n) return false;
    if (!in_win) {
      h = h2;
      hb = at;
    }
    uint32_t offset = (uint32_t)(h >> (8 * (at - hb))) & 0xffffu;
    ip += 2;
    if (ml == 19 && !lz4_ext_win(in, n, h, hb, ip, ml, cap - op)) return false;
    if (offset == 0 || offset > op + dict.len() || ml > cap - op) return false;
    if (offset > op) { // never without a dictionary
      uint32_t c = lz4_dict_part(dict, out, op, offset, ml);
      op += c;
      ml -= c;
      if (ml == 0) continue;
    }
    uint32_t src = op - offset;
    uint32_t end = op + ml;
    if (offset >= 16) {
      for (uint32_t i = 0; i < ml; i += 16) {
        uint64_t a = lds_ld64(out + src + i);
        uint64_t b = lds_ld64(out + src + i + 8);
        lds_st64(out + op + i, a);
        lds_st64(out + op + i + 8, b);
      }
    } else if (offset >= 8) {
      for (uint32_t i = 0; i < ml; i += 8)
        lds_st64(out + op + i, lds_ld64(out + src + i));
    } else {
      // pattern doubling: each 8-B store makes (op - src) more bytes valid
      // and doubles the usable distance; what a load takes from beyond the
      // valid point lands beyond the advancing store point and is
      // overwritten by the next round
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
  }
  return op == cap;
}

#endif // DCW_LZ4_LDS

// Generic byte-exact form: touches in[0, n) and out[0, cap) only.  The GPU
// uses it global to global for blocks beyond DEC_MAX; the host uses the
// same function (index blocks in parse_sst).
template <class D = Lz4NoDict>
DCW_LZ4_FN bool lz4_dec(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap,
                        const D& dict = D()) {
  if ((n | cap) >> 31) return false; // keeps the 32-bit length sums exact
  uint32_t ip = 0, op = 0;
  while (ip < n) {
    uint32_t tok = in[ip++];
    uint32_t ll = tok >> 4, ml = (tok & 15) + 4;
    if (ll == 15) {
      uint32_t b;
      do {
        if (ip >= n) return false;
        b = in[ip++];
        ll += b;
        if (ll > n - ip) return false;
      } while (b == 255);
    }
    if (ll > n - ip || ll > cap - op) return false;
    uint32_t i = 0;
    for (; i + 8 <= ll; i += 8) {
      uint64_t v;
      memcpy(&v, in + ip + i, 8);
      memcpy(out + op + i, &v, 8);
    }
    for (; i < ll; i++) out[op + i] = in[ip + i];
    ip += ll;
    op += ll;
    if (ip == n) break;
    if (ip + 2 > n) return false;
    uint32_t offset = (uint32_t)in[ip] | ((uint32_t)in[ip + 1] << 8);
    ip += 2;
    if (ml == 19) {
      uint32_t b;
      do {
        if (ip >= n) return false;
        b = in[ip++];
        ml += b;
        if (ml > cap - op) return false;
      } while (b == 255);
    }
    if (offset == 0 || offset > op + dict.len() || ml > cap - op) return false;
    if (offset > op) { // never without a dictionary
      uint32_t c = lz4_dict_part(dict, out, op, offset, ml);
      op += c;
      ml -= c;
    }
    const uint8_t* s = out + op - offset;
    i = 0;
    if (offset >= 8)
      for (; i + 8 <= ml; i += 8) {
        uint64_t v;
        memcpy(&v, s + i, 8);
        memcpy(out + op + i, &v, 8);
      }
    for (; i < ml; i++) out[op + i] = s[i];
    op += ml;
  }
  return op == cap;
}

} // namespace dcw
