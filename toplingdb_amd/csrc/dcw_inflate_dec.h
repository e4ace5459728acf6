// dcw_inflate_dec.h — deflate (RFC 1951) decoders for input data blocks of
// type 2 (kZlibCompression).  Included by dcw_k_decode.h (zlib_preamble for
// k_verify_usize), by dcw_zlib.hip for the GPU (k_decompress_zlib), by
// dcw_host.cpp (inflate_dec for index blocks in parse_sst) and by
// tools/zlib_host, which runs the wave decoder on the CPU in the kernel's
// schedule.  Plain C++; the wave primitives (lane loop, barrier) are macros
// with a device and a host form, as in dcw_zstd_dec.h.
//
// A stored block is varint32(decoded size) + one raw deflate stream: no zlib
// or gzip header, no Adler-32 (compress_format_version 2, window_bits -14).
//
// Acceptance rule, the same for inflate_dec and infl_dec_wave.  Every point
// is a bounds decision taken before the move it guards.  A stream is
// accepted iff
//   - every block header is valid: BTYPE 3 is refused;
//   - a stored block's LEN equals ~NLEN and its bytes lie inside the input;
//   - a dynamic block has HLIT <= 286 and HDIST <= 30;
//   - the code-length code, the literal/length code and the distance code are
//     neither over-subscribed nor incomplete, with two exceptions for the
//     distance code: a single symbol of length 1 (zlib's exception), and no
//     symbol at all (RFC 1951 3.2.7: the data is all literals; zlib builds
//     such a table as well and refuses only a distance that uses it, as here);
//   - no repeat code runs past HLIT + HDIST, no code 16 stands at position 0;
//   - symbol 256 has a code;
//   - literal/length symbols 286, 287 and distance symbols 30, 31 do not occur;
//   - every distance is <= the bytes produced so far (so <= 32768 by format);
//   - the final block's end-of-block is reached with exactly `cap` bytes
//     produced, and no store ever goes past `cap`;
//   - no bit is read beyond the input: the bit reader feeds zeros behind the
//     last byte and counts them, and a symbol that used one is refused;
//   - bytes left over behind the final block are no error (Zlib_Uncompress
//     does not look at avail_in either);
//   - n < 2^28 and cap < 2^31, which keeps the 32-bit positions exact.
// This is stricter than zlib in one place (zlib accepts a literal/length code
// of a single 1-bit symbol) and never laxer.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IHD __host__ __device__ inline
#else
#define IHD static inline
#endif

namespace dcw {

// varint32 preamble of a stored type-2 block: bytes consumed, or -1 for a
// preamble that is cut short or still continues after 5 bytes
IHD int zlib_preamble(const uint8_t* p, uint32_t n, uint32_t* usize) {
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

// length symbol 257..285 and distance symbol 0..29: base value and extra bits
IHD uint32_t infl_len_extra(uint32_t s) { return s < 265 || s == 285 ? 0 : (s - 261) >> 2; }
IHD uint32_t infl_len_base(uint32_t s) {
  if (s < 265) return s - 254;
  if (s == 285) return 258;
  return 3 + ((4 + ((s - 265) & 3)) << ((s - 261) >> 2));
}
IHD uint32_t infl_dist_extra(uint32_t d) { return d < 4 ? 0 : (d >> 1) - 1; }
IHD uint32_t infl_dist_base(uint32_t d) {
  return d < 4 ? d + 1 : 1 + ((2 + (d & 1)) << ((d >> 1) - 1));
}
// where the i-th code-length-code length goes: 16 17 18 0 8 7 9 6 10 5 11 4
// 12 3 13 2 14 1 15, five bits each
IHD uint32_t infl_cl_order(uint32_t i) {
  const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 |
                      7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                      5ull << 45 | 11ull << 50 | 4ull << 55;
  const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 |
                      1ull << 25 | 15ull << 30;
  return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}
// length of a fixed block's literal/length symbol
IHD uint32_t infl_fixed_len(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

// ------------------------------------------------------------ serial decoder
// One bit and one code length at a time, canonical: slow and plain.  The
// host's decoder for index blocks and the wave decoder's referee in
// tools/zlib_host.  Touches in[0, n) and out[0, cap) only.
struct InflSerial {
  const uint8_t* in;
  uint32_t n, ip, buf, cnt;
  bool over;
};
IHD uint32_t infl_s_bits(InflSerial& s, uint32_t need) {
  while (s.cnt < need) {
    if (s.ip >= s.n) {
      s.over = true;
      return 0;
    }
    s.buf |= (uint32_t)s.in[s.ip++] << s.cnt;
    s.cnt += 8;
  }
  uint32_t v = s.buf & ((1u << need) - 1);
  s.buf >>= need;
  s.cnt -= need;
  return v;
}
struct InflSerialCode {
  uint16_t count[16], symbol[288];
};
// Kraft remainder: 0 complete, > 0 incomplete, < 0 over-subscribed
IHD int infl_s_build(InflSerialCode& h, const uint8_t* lens, uint32_t nsym) {
  uint16_t offs[16];
  for (uint32_t l = 0; l < 16; l++) h.count[l] = 0;
  for (uint32_t s = 0; s < nsym; s++) h.count[lens[s]]++;
  int left = 1;
  for (uint32_t l = 1; l < 16; l++) {
    left = left * 2 - (int)h.count[l];
    if (left < 0) return left;
  }
  offs[1] = 0;
  for (uint32_t l = 1; l < 15; l++) offs[l + 1] = offs[l] + h.count[l];
  for (uint32_t s = 0; s < nsym; s++)
    if (lens[s]) h.symbol[offs[lens[s]]++] = (uint16_t)s;
  return left;
}
IHD int infl_s_sym(InflSerial& s, const InflSerialCode& h) {
  int code = 0, first = 0, index = 0;
  for (uint32_t l = 1; l < 16; l++) {
    code |= (int)infl_s_bits(s, 1);
    if (s.over) return -1;
    int c = h.count[l];
    if (code - c < first) return h.symbol[index + (code - first)];
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -1; // no code of any length: an incomplete code was used
}
IHD bool infl_dist_code_ok(int left, const uint16_t* count) {
  uint32_t used = 0;
  for (uint32_t l = 1; l < 16; l++) used += count[l];
  return left == 0 || (left > 0 && (used == 0 || (used == 1 && count[1] == 1)));
}

IHD bool inflate_dec(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap) {
  if ((n >> 28) || (cap >> 31)) return false;
  InflSerial s = {in, n, 0, 0, 0, false};
  InflSerialCode ll, dd;
  uint8_t lens[320];
  uint32_t op = 0, last;
  do {
    last = infl_s_bits(s, 1);
    uint32_t type = infl_s_bits(s, 2);
    if (s.over || type == 3) return false;
    if (type == 0) {
      s.buf = 0;
      s.cnt = 0; // the rest of the byte
      uint32_t len = infl_s_bits(s, 16), nlen = infl_s_bits(s, 16);
      if (s.over || len != (~nlen & 0xffffu)) return false;
      if (len > n - s.ip || len > cap - op) return false;
      memcpy(out + op, in + s.ip, len);
      s.ip += len;
      op += len;
      continue;
    }
    if (type == 1) {
      for (uint32_t i = 0; i < 288; i++) lens[i] = (uint8_t)infl_fixed_len(i);
      for (uint32_t i = 0; i < 32; i++) lens[288 + i] = 5;
      infl_s_build(ll, lens, 288);
      infl_s_build(dd, lens + 288, 32);
    } else {
      uint32_t hlit = infl_s_bits(s, 5) + 257, hdist = infl_s_bits(s, 5) + 1;
      uint32_t hclen = infl_s_bits(s, 4) + 4;
      if (s.over || hlit > 286 || hdist > 30) return false;
      for (uint32_t i = 0; i < 19; i++) lens[i] = 0;
      for (uint32_t i = 0; i < hclen; i++) lens[infl_cl_order(i)] = (uint8_t)infl_s_bits(s, 3);
      if (s.over || infl_s_build(ll, lens, 19) != 0) return false;
      uint32_t i = 0, tot = hlit + hdist;
      while (i < tot) {
        int sym = infl_s_sym(s, ll);
        if (sym < 0) return false;
        if (sym < 16) {
          lens[i++] = (uint8_t)sym;
          continue;
        }
        uint32_t val = 0, rep;
        if (sym == 16) {
          if (i == 0) return false;
          val = lens[i - 1];
          rep = 3 + infl_s_bits(s, 2);
        } else if (sym == 17) {
          rep = 3 + infl_s_bits(s, 3);
        } else {
          rep = 11 + infl_s_bits(s, 7);
        }
        if (s.over || rep > tot - i) return false;
        while (rep--) lens[i++] = (uint8_t)val;
      }
      if (lens[256] == 0) return false;
      uint8_t dl[32];
      memcpy(dl, lens + hlit, hdist);
      if (infl_s_build(ll, lens, hlit) != 0) return false;
      if (!infl_dist_code_ok(infl_s_build(dd, dl, hdist), dd.count)) return false;
    }
    for (;;) {
      int sym = infl_s_sym(s, ll);
      if (sym < 0) return false;
      if (sym < 256) {
        if (op >= cap) return false;
        out[op++] = (uint8_t)sym;
        continue;
      }
      if (sym == 256) break;
      if (sym > 285) return false;
      uint32_t len = infl_len_base(sym) + infl_s_bits(s, infl_len_extra(sym));
      int ds = infl_s_sym(s, dd);
      if (ds < 0 || ds > 29) return false;
      uint32_t dist = infl_dist_base(ds) + infl_s_bits(s, infl_dist_extra(ds));
      if (s.over || dist > op || len > cap - op) return false;
      for (uint32_t i = 0; i < len; i++) out[op + i] = out[op + i - dist];
      op += len;
    }
  } while (!last);
  return op == cap;
}

#if defined(__HIPCC__)
// dcw_zlib.hip: k_decompress_zlib over `list`, one work-group of one wave per
// grid entry
void launch_decompress_zlib(uint32_t grid, hipStream_t stream, const uint8_t* blob,
                            const uint64_t* boff, const uint32_t* bsize,
                            const uint64_t* uoff, const uint32_t* usize,
                            const uint32_t* list, uint32_t nlist, uint8_t* ublob,
                            uint32_t* err_flag, uint32_t err_code);
#endif

#ifdef DCW_INFLATE_WAVE
// ---------------------------------------------------------------- wave form
// One wave decodes one stream.  The code is a sequence of phases: `IW_LANES
// { ... }` is the body one lane runs (on the host a loop over the 64 lanes,
// ascending or descending), IW_SYNC() separates phases that communicate
// through the InflLds or through the output.  Control flow between phases
// depends only on InflLds fields read after a sync, so it is uniform.
//   lane 0      block headers; the literal/length and distance code lengths
//               of a dynamic block (the repeat codes make that serial); the
//               symbol walk: a 64-bit bit buffer refilled by 8-byte loads,
//               literals stored where they belong, each length/distance pair
//               recorded in a batch of up to 64 matches
//   lane i      the i-th code-length-code length, read at its fixed position
//   all lanes   the decode tables (lane 16g + L counts and then sorts the
//               symbols of length L of code g; every lane fills the
//               replicated primary entries of its symbols); the matches of a
//               batch, one per lane, in dependency rounds; stored blocks
// Decode tables: a primary table indexed by the next P stream bits, P = 10
// for literal/length, 8 for distance, 7 for the code-length code; an entry is
// symbol | length << 9, 0 where no code of up to P bits matches.  Deflate
// packs a code most significant bit first into a stream that is read least
// significant bit first, so the index is the bit-reversed code.  A longer
// code is resolved canonically: the bit-reversed 15-bit peek, cut to each
// length L in P+1..15, is a code of that length iff it lies in
// [first[L], first[L] + count[L]); its symbol is sorted[offs[L] + code -
// first[L]].  No second-level tables: 2 KiB + 512 B + 256 B of primaries.
//
// Memory policy: `M` gives the stream (in) and the output (out).  InflMemLds: both staged
// in LDS by the kernel (n, cap <= kInflMax).  InflMemGlobal: the stream where
// it was staged in global memory, the output the block's slot of the decoded
// blob; a match then reads back what the wave stored earlier, and between the
// store and the load lies an IW_SYNC(), whose fence and wait for outstanding
// stores make the bytes visible to the other lanes of the wave (they share
// the compute unit's vector cache), as in dcw_zstd_dec_large.h.  Neither
// policy reads or writes a byte outside in[0, n) and out[0, cap).
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
#define IFN __device__ __forceinline__
#define IW_LANES for (uint32_t lane = zlane, ionce = 1; ionce; ionce = 0)
#define IW_SYNC()                                          \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); \
    __builtin_amdgcn_s_waitcnt(0);                         \
    __builtin_amdgcn_wave_barrier();                       \
  } while (0)
#define ISTAT_MAX(i, v) ((void)0)
#define ISTAT(i) ((void)0)
#else
#define IFN static inline
static int iw_descending = 0; // the host runs every stream in both lane orders
#define IW_LANES \
  for (uint32_t ii = 0, lane = iw_descending ? 63 : 0; ii < 64; \
       ii++, lane = iw_descending ? 63 - ii : ii)
#define IW_SYNC() ((void)0)
enum InflStat { IS_STORED, IS_FIXED, IS_DYNAMIC, IS_MAXLEN, IS_ROUNDS, IS_FIXED_BUILDS, IS_COUNT };
static uint32_t istat[IS_COUNT];
#define ISTAT(i) (istat[i]++)
#define ISTAT_MAX(i, v) (istat[i] = istat[i] < (v) ? (v) : istat[i])
#endif

static const uint32_t kInflMax = 4992; // == DEC_MAX (dcw_k_decode.h)
static const uint32_t kInflPL = 10, kInflPD = 8, kInflPC = 7;
static const uint32_t kInflBatch = 64;

// canonical code: symbols per length, first code and first slot in `sorted`
// of each length, symbols with a code
struct InflCode {
  uint16_t count[16], first[16], offs[16];
  uint32_t used;
};
// codes 0 / 1 / 2: literal/length, distance, code-length
struct alignas(16) InflLds {
  uint16_t tabLL[1u << kInflPL], tabD[1u << kInflPD], tabCL[1u << kInflPC];
  uint16_t sortLL[288], sortD[32], sortCL[24];
  alignas(8) uint8_t lensLL[288];
  alignas(8) uint8_t lensD[32];
  alignas(8) uint8_t lensCL[24];
  InflCode code[3];
  uint64_t bmask[kInflBatch]; // earlier matches of the batch that a match reads
  uint32_t bdst[kInflBatch];  // where a match goes
  uint32_t bld[kInflBatch];   // its length | distance << 9
  alignas(8) uint8_t bfin[kInflBatch];
  uint32_t fail, last, btype, hlit, hdist, hclen, blk_bit, nb, eob;
  uint32_t tfixed; // the tables hold the fixed code
  uint32_t st_src, st_dst, st_len;
};

struct InflMemLds {
  const uint8_t* in;
  uint8_t* out;
};
struct InflMemGlobal {
  const uint8_t* in;
  uint8_t* out;
};

// two 32-bit moves: any alignment, and in LDS the widest move that does not
// fall apart into byte moves (dcw_snap_dec_lds.h)
IFN uint64_t infl_ld64(const uint8_t* p) {
  uint32_t lo, hi;
  memcpy(&lo, p, 4);
  memcpy(&hi, p + 4, 4);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
IFN void infl_st64(uint8_t* p, uint64_t v) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  memcpy(p, &lo, 4);
  memcpy(p + 4, &hi, 4);
}
IFN uint32_t infl_rev15(uint32_t x) { // x < 2^15
#if defined(__HIP_DEVICE_COMPILE__)
  return __brev(x) >> 17;
#else
  x = ((x & 0x5555u) << 1) | ((x >> 1) & 0x5555u);
  x = ((x & 0x3333u) << 2) | ((x >> 2) & 0x3333u);
  x = ((x & 0x0f0fu) << 4) | ((x >> 4) & 0x0f0fu);
  x = ((x & 0x00ffu) << 8) | ((x >> 8) & 0x00ffu);
  return x >> 1;
#endif
}

// Lane 0's bit reader.  `bb` holds `bc` unread bits, lowest first; `ip` is
// the next byte to fetch.  Behind the last byte of the input the reader
// feeds zero bytes and counts their bits in `virt`: bits of the input are
// left iff bc >= virt, which infl_over() asks after every symbol.
struct InflBits {
  uint64_t bb;
  uint32_t bc, ip, virt;
};
// at least 56 bits afterwards
IFN void infl_refill(InflBits& b, const uint8_t* in, uint32_t n) {
  if (b.ip + 8 <= n) { // whole window inside the input: one fetch
    b.bb |= infl_ld64(in + b.ip) << b.bc;
    b.ip += (63 - b.bc) >> 3;
    b.bc |= 56;
    return;
  }
  while (b.bc < 56) {
    uint64_t v = 0;
    if (b.ip < n) v = in[b.ip]; else b.virt += 8;
    b.bb |= v << b.bc;
    b.ip++;
    b.bc += 8;
  }
}
IFN void infl_drop(InflBits& b, uint32_t k) {
  b.bb >>= k;
  b.bc -= k;
}
IFN bool infl_over(const InflBits& b) { return b.bc < b.virt; }

IFN uint16_t* infl_tab(InflLds& S, uint32_t t) { return t == 0 ? S.tabLL : t == 1 ? S.tabD : S.tabCL; }
IFN uint16_t* infl_sorted(InflLds& S, uint32_t t) { return t == 0 ? S.sortLL : t == 1 ? S.sortD : S.sortCL; }
IFN uint8_t* infl_lens(InflLds& S, uint32_t t) { return t == 0 ? S.lensLL : t == 1 ? S.lensD : S.lensCL; }
IFN uint32_t infl_p(uint32_t t) { return t == 0 ? kInflPL : t == 1 ? kInflPD : kInflPC; }
IFN uint32_t infl_nsym(uint32_t t) { return t == 0 ? 288 : t == 1 ? 32 : 24; }

// The decode tables out of the code lengths in lensLL and lensD (both = 1)
// or lensCL (both = 0); lengths behind the code's last symbol are 0.  Sets
// S.fail for a code the acceptance rule refuses.
IFN bool infl_build(InflLds& S, uint32_t both, uint32_t zlane) {
  const uint32_t t0 = both ? 0 : 2, nt = both ? 2 : 1;
  IW_LANES { // clear the primaries; lane 16g + L counts the symbols of length L
    for (uint32_t t = t0; t < t0 + nt; t++) {
      uint16_t* tab = infl_tab(S, t);
      for (uint32_t i = lane; i < (1u << infl_p(t)); i += 64) tab[i] = 0;
    }
    const uint32_t g = lane >> 4, L = lane & 15;
    if (g < nt) {
      const uint8_t* lens = infl_lens(S, t0 + g);
      uint32_t c = 0;
      for (uint32_t w = 0; w < infl_nsym(t0 + g); w += 8) {
        uint64_t v;
        memcpy(&v, lens + w, 8);
        for (uint32_t k = 0; k < 8; k++) c += ((v >> (8 * k)) & 0xff) == L;
      }
      S.code[t0 + g].count[L] = (uint16_t)c;
    }
  }
  IW_SYNC();
  IW_LANES { // Kraft sum, first code and first slot of each length
    const uint32_t g = lane >> 4;
    if ((lane & 15) == 0 && g < nt) {
      InflCode& C = S.code[t0 + g];
      int32_t left = 1;
      uint32_t code = 0, off = 0, prev = 0, maxlen = 0;
      for (uint32_t L = 1; L < 16; L++) {
        const uint32_t c = C.count[L];
        if (left >= 0) left = left * 2 - (int32_t)c;
        code = (code + prev) << 1;
        C.first[L] = (uint16_t)code;
        C.offs[L] = (uint16_t)off;
        off += c;
        prev = c;
        if (c) maxlen = L;
      }
      C.used = off;
      bool ok = left == 0;
      if (t0 + g == 1 && left > 0) ok = off == 0 || (off == 1 && C.count[1] == 1);
      if (t0 + g == 0 && S.lensLL[256] == 0) ok = false;
      if (!ok) S.fail = 1;
      if (both) ISTAT_MAX(IS_MAXLEN, maxlen);
      (void)maxlen;
    }
  }
  IW_SYNC();
  if (S.fail) return false;
  IW_LANES { // counting sort by (length, symbol): lane 16g + L places its own
    const uint32_t g = lane >> 4, L = lane & 15;
    if (g < nt && L) {
      const uint8_t* lens = infl_lens(S, t0 + g);
      uint16_t* sorted = infl_sorted(S, t0 + g);
      uint32_t o = S.code[t0 + g].offs[L];
      for (uint32_t w = 0; w < infl_nsym(t0 + g); w += 8) {
        uint64_t v;
        memcpy(&v, lens + w, 8);
        for (uint32_t k = 0; k < 8; k++)
          if (((v >> (8 * k)) & 0xff) == L) sorted[o++] = (uint16_t)(w + k);
      }
    }
  }
  IW_SYNC();
  IW_LANES { // a lane per symbol: every primary entry its code is a prefix of
    for (uint32_t t = t0; t < t0 + nt; t++) {
      const InflCode& C = S.code[t];
      const uint8_t* lens = infl_lens(S, t);
      const uint16_t* sorted = infl_sorted(S, t);
      uint16_t* tab = infl_tab(S, t);
      const uint32_t P = infl_p(t), used = C.used;
      for (uint32_t k = lane; k < used; k += 64) {
        const uint32_t sym = sorted[k], L = lens[sym];
        if (L > P) continue;
        const uint32_t code = C.first[L] + (k - C.offs[L]);
        for (uint32_t i = infl_rev15(code) >> (15 - L); i < (1u << P); i += 1u << L)
          tab[i] = (uint16_t)(sym | L << 9);
      }
    }
  }
  IW_SYNC();
  return true;
}

// the symbol at the head of the bit buffer (>= 15 bits valid): symbol |
// length << 9, or 0 where the bits are no code
IFN uint32_t infl_sym(const InflLds& S, uint32_t t, const uint16_t* tab,
                      const uint16_t* sorted, uint32_t P, uint64_t bb) {
  uint32_t e = tab[(uint32_t)bb & ((1u << P) - 1)];
  if (e) return e;
  const InflCode& C = S.code[t];
  const uint32_t c15 = infl_rev15((uint32_t)bb & 0x7fffu);
  for (uint32_t L = P + 1; L < 16; L++) {
    const uint32_t d = (c15 >> (15 - L)) - C.first[L];
    if (d < C.count[L]) return sorted[C.offs[L] + d] | L << 9;
  }
  return 0;
}

// A batch of matches: lane j copies match j once every earlier match of the
// batch whose destination meets its source has been copied.  The lowest
// unfinished match never waits, so every round finishes at least one.
template <class M>
IFN void infl_exec_batch(InflLds& S, const M& m, uint32_t nb, uint32_t zlane) {
  uint8_t* out = m.out;
  IW_LANES {
    uint64_t mask = 0;
    if (lane < nb) {
      const uint32_t d = S.bdst[lane], ld = S.bld[lane];
      const uint32_t s0 = d - (ld >> 9), s1 = s0 + (ld & 511);
      for (uint32_t k = 0; k < lane; k++) { // S.bdst[k]: one address, a broadcast
        const uint32_t dk = S.bdst[k], ek = dk + (S.bld[k] & 511);
        if (dk < s1 && s0 < ek) mask |= 1ull << k;
      }
    }
    S.bmask[lane] = mask;
    S.bfin[lane] = lane >= nb;
  }
  IW_SYNC();
  uint32_t rounds = 0;
  for (;;) {
    uint64_t done = 0; // uniform: the lanes that have finished
    for (uint32_t w = 0; w < 8; w++) {
      uint64_t v;
      memcpy(&v, S.bfin + 8 * w, 8);
      done |= ((v * 0x0102040810204080ull) >> 56) << (8 * w);
    }
    if (done == ~0ull) break;
    rounds++;
    IW_LANES {
      if (((done >> lane) & 1) || (S.bmask[lane] & ~done)) continue;
      const uint32_t d = S.bdst[lane], ld = S.bld[lane];
      const uint32_t dist = ld >> 9, len = ld & 511;
      uint8_t* q = out + d;
      const uint8_t* s = q - dist;
      uint32_t i = 0;
      // dist >= 8: an 8-byte load ends at or below the store it feeds, and
      // where dist < len it reads what this lane stored before it
      if (dist >= 8)
        for (; i + 8 <= len; i += 8) infl_st64(q + i, infl_ld64(s + i));
      for (; i < len; i++) q[i] = s[i]; // the period, byte by byte
      S.bfin[lane] = 1;
    }
    IW_SYNC();
  }
  ISTAT_MAX(IS_ROUNDS, rounds);
  (void)rounds;
}

// The stream m.in[0, n) -> m.out[0, cap).
template <class M>
IFN bool infl_dec_wave(InflLds& S, const M& m, uint32_t n, uint32_t cap,
                       uint32_t zlane) {
  const uint8_t* in = m.in;
  uint8_t* out = m.out;
  InflBits b = {0, 0, 0, 0}; // lane 0's
  uint32_t op = 0;           // lane 0's: bytes produced
  IW_LANES {
    if (lane == 0) {
      S.fail = (n >> 28) || (cap >> 31);
      S.last = 0;
    }
  }
  IW_SYNC();
  if (S.fail) return false;
  do {
    IW_LANES { // block header
      if (lane == 0) {
        infl_refill(b, in, n);
        S.blk_bit = b.ip * 8 - b.bc;
        S.last = (uint32_t)b.bb & 1;
        const uint32_t type = ((uint32_t)b.bb >> 1) & 3;
        S.btype = type;
        infl_drop(b, 3);
        if (type == 3) S.fail = 1;
        if (type == 2) {
          S.hlit = ((uint32_t)b.bb & 31) + 257;
          S.hdist = (((uint32_t)b.bb >> 5) & 31) + 1;
          S.hclen = (((uint32_t)b.bb >> 10) & 15) + 4;
          infl_drop(b, 14);
          if (S.hlit > 286 || S.hdist > 30) S.fail = 1;
        } else if (type == 0) { // the rest of the byte, LEN, NLEN
          infl_drop(b, b.bc & 7);
          infl_refill(b, in, n);
          const uint32_t len = (uint32_t)b.bb & 0xffffu;
          const uint32_t nlen = ((uint32_t)(b.bb >> 16)) & 0xffffu;
          infl_drop(b, 32);
          if (!infl_over(b)) {
            const uint32_t src = b.ip - b.bc / 8; // bytes in the buffer go back
            if (len != (~nlen & 0xffffu) || len > n - src || len > cap - op) S.fail = 1;
            S.st_src = src;
            S.st_dst = op;
            S.st_len = len;
            op += len;
            b = InflBits{0, 0, src + len, 0};
          }
        }
        if (infl_over(b)) S.fail = 1;
      }
    }
    IW_SYNC();
    if (S.fail) return false;
    const uint32_t btype = S.btype;
    if (btype == 0) { // a copy by the wave, 16 bytes per lane and step
      ISTAT(IS_STORED);
      const uint8_t* s = in + S.st_src;
      uint8_t* d = out + S.st_dst;
      const uint32_t len = S.st_len;
      IW_LANES {
        for (uint32_t t = lane * 16; t + 16 <= len; t += 64 * 16) {
          infl_st64(d + t, infl_ld64(s + t));
          infl_st64(d + t + 8, infl_ld64(s + t + 8));
        }
        const uint32_t t = (len & ~15u) + lane;
        if (lane < 16 && t < len) d[t] = s[t];
      }
      IW_SYNC();
      continue;
    }
    if (btype == 2) {
      ISTAT(IS_DYNAMIC);
      const uint32_t hclen = S.hclen, blk_bit = S.blk_bit;
      IW_LANES { // lane i: the i-th code-length-code length, bit 17 + 3i
        if (lane < 19) {
          uint32_t v = 0;
          if (lane < hclen) {
            const uint32_t at = blk_bit + 17 + 3 * lane, by = at >> 3;
            if (at + 3 > 8 * n) {
              S.fail = 1;
            } else {
              uint32_t w = in[by];
              if (by + 1 < n) w |= (uint32_t)in[by + 1] << 8;
              v = (w >> (at & 7)) & 7;
            }
          }
          S.lensCL[infl_cl_order(lane)] = (uint8_t)v;
        } else if (lane < 24) {
          S.lensCL[lane] = 0;
        }
        for (uint32_t i = lane; i < 288; i += 64) S.lensLL[i] = 0;
        if (lane < 32) S.lensD[lane] = 0;
      }
      IW_SYNC();
      if (S.fail || !infl_build(S, 0, zlane)) return false;
      IW_LANES { // the HLIT + HDIST code lengths
        if (lane == 0) {
          S.tfixed = 0;
          for (uint32_t rem = 3 * hclen; rem;) {
            const uint32_t k = rem < 32 ? rem : 32;
            infl_refill(b, in, n);
            infl_drop(b, k);
            rem -= k;
          }
          const uint32_t hlit = S.hlit, tot = hlit + S.hdist;
          uint32_t i = 0, prev = 0;
          bool bad = false;
          while (i < tot && !bad) {
            infl_refill(b, in, n);
            const uint32_t e = S.tabCL[(uint32_t)b.bb & ((1u << kInflPC) - 1)];
            if (!e) { bad = true; break; }
            infl_drop(b, e >> 9);
            const uint32_t sym = e & 511;
            uint32_t rep = 1, val = sym;
            if (sym == 16) {
              if (i == 0) { bad = true; break; }
              val = prev;
              rep = 3 + ((uint32_t)b.bb & 3);
              infl_drop(b, 2);
            } else if (sym == 17) {
              val = 0;
              rep = 3 + ((uint32_t)b.bb & 7);
              infl_drop(b, 3);
            } else if (sym == 18) {
              val = 0;
              rep = 11 + ((uint32_t)b.bb & 127);
              infl_drop(b, 7);
            }
            if (infl_over(b) || rep > tot - i) { bad = true; break; }
            for (; rep; rep--, i++) {
              if (i < hlit) S.lensLL[i] = (uint8_t)val;
              else S.lensD[i - hlit] = (uint8_t)val;
            }
            prev = val;
          }
          if (bad) S.fail = 1;
        }
      }
      IW_SYNC();
      if (S.fail || !infl_build(S, 1, zlane)) return false;
    } else {
      ISTAT(IS_FIXED);
      if (!S.tfixed) { // a run of fixed blocks builds once
        ISTAT(IS_FIXED_BUILDS);
        IW_LANES {
          for (uint32_t i = lane; i < 288; i += 64) S.lensLL[i] = (uint8_t)infl_fixed_len(i);
          if (lane < 32) S.lensD[lane] = 5;
        }
        IW_SYNC();
        if (!infl_build(S, 1, zlane)) return false;
        IW_LANES { if (lane == 0) S.tfixed = 1; }
        IW_SYNC();
      }
    }
    for (;;) { // the symbols of the block, a batch of matches at a time
      IW_LANES {
        if (lane == 0) {
          uint32_t nb = 0, eob = 0;
          bool bad = false;
          while (nb < kInflBatch) {
            infl_refill(b, in, n);
            uint32_t e = infl_sym(S, 0, S.tabLL, S.sortLL, kInflPL, b.bb);
            if (!e) { bad = true; break; }
            infl_drop(b, e >> 9);
            uint32_t sym = e & 511;
            if (sym < 256) {
              if (infl_over(b) || op >= cap) { bad = true; break; }
              out[op++] = (uint8_t)sym;
              continue;
            }
            if (sym == 256) {
              bad = infl_over(b);
              eob = 1;
              break;
            }
            if (sym > 285) { bad = true; break; }
            uint32_t x = infl_len_extra(sym);
            const uint32_t len = infl_len_base(sym) + ((uint32_t)b.bb & ((1u << x) - 1));
            infl_drop(b, x);
            e = infl_sym(S, 1, S.tabD, S.sortD, kInflPD, b.bb);
            if (!e) { bad = true; break; }
            infl_drop(b, e >> 9);
            sym = e & 511;
            if (sym > 29) { bad = true; break; }
            x = infl_dist_extra(sym);
            const uint32_t dist = infl_dist_base(sym) + ((uint32_t)b.bb & ((1u << x) - 1));
            infl_drop(b, x);
            if (infl_over(b) || dist > op || len > cap - op) { bad = true; break; }
            S.bdst[nb] = op;
            S.bld[nb] = len | dist << 9;
            nb++;
            op += len;
          }
          S.nb = bad ? 0 : nb;
          S.eob = eob;
          if (bad) S.fail = 1;
        }
      }
      IW_SYNC();
      if (S.fail) return false;
      if (S.nb) infl_exec_batch(S, m, S.nb, zlane);
      if (S.eob) break;
    }
  } while (!S.last);
  IW_LANES { if (lane == 0 && op != cap) S.fail = 1; }
  IW_SYNC();
  return !S.fail;
}
#endif // DCW_INFLATE_WAVE

} // namespace dcw
