// dcw_zstd_dec.h — Zstandard frame decoder for input data blocks of type 7.
// Included by dcw_k_decode.h for the GPU (k_decompress_zstd), by
// dcw_worker.cpp for the eligibility walk and by tools/zstd_host, which runs
// the wave decoder on the CPU in the kernel's schedule.  Plain C++; the few
// wave primitives (lane loop, barrier, prefix sum) are macros with a device
// and a host form.
//
// A stored block is varint32(decoded size) + one zstd frame (RFC 8878).  The
// decoder takes frames without dictionary and without content checksum whose
// stored and decoded sizes are both within kZstdMax: zstd_eligible() says
// which blocks those are, everything else stays on the host path.
//
// One wave decodes one frame out of a ZstdWave (LDS on the device).  The code
// is a sequence of PHASES: `ZW_LANES { ... }` is the body one lane runs
// (on the host: a loop over the 64 lanes, ascending or descending), and
// ZW_SYNC() separates phases that communicate through the ZstdWave.  Control
// flow between phases depends only on ZstdWave fields read after a sync, so
// it is uniform across the wave.  Who does what:
//   lane 0      frame, block, literals and sequences headers; FSE table
//               descriptions; the Huffman weights; the sequence bitstream,
//               64 sequences at a time
//   all lanes   FSE decode tables (each lane places a slice of the spread's
//               visit order after a prefix sum of skipped positions, then
//               one lane per symbol numbers its cells in table order);
//               the Huffman decode table (one lane per weight lays the
//               symbols out, then each lane fills a slice of the table);
//               literal runs of a batch (one run per lane, positions from a
//               prefix sum of ll and ll+ml); every match, in sequence order,
//               64 bytes per step; raw/RLE blocks and trailing literals
//   lanes 0..3  the four Huffman streams of 4-stream literals
//
// Refusals are decisions taken before any move; a refused frame leaves
// `fail` set.  Where libzstd 1.4.8 is laxer than the format (an over-read
// sequence bitstream, a resolved offset of 0, Huffman table log 12) this
// decoder refuses; it never accepts what libzstd refuses.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZHD __host__ __device__ inline
#else
#define ZHD static inline
#endif

namespace dcw {

static const uint32_t kZstdMax = 4992; // == DEC_MAX (dcw_k_decode.h)
static const uint32_t kZstdPad = 16;   // slack for the 8-byte bit fetches
static const uint32_t kZstdMagic = 0xFD2FB528u;
static const uint32_t kZstdBlockMax = 128u << 10; // Block_Maximum_Size

ZHD int zstd_preamble(const uint8_t* p, uint32_t n, uint32_t* usize) {
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

// The eligibility walk over a stored type-7 block: preamble, magic, no
// dictionary ID, no content checksum, reserved bit clear, the block headers
// chain exactly to the end of the payload as one frame, stored and promised
// size within kZstdMax.  Touches p[0, n) only.  `dict`: the block's file has a
// dictionary (dcw_zstd_dict.h), so a Dictionary_ID field of 1, 2 or 4 bytes
// may stand behind the window descriptor.
ZHD uint32_t zstd_did_bytes(uint32_t fhd) { return (fhd & 3) == 3 ? 4 : fhd & 3; }
ZHD bool zstd_eligible(const uint8_t* p, uint32_t n, bool dict = false) {
  uint32_t un;
  int hn = zstd_preamble(p, n, &un);
  if (hn < 0 || un > kZstdMax || n - (uint32_t)hn > kZstdMax) return false;
  p += hn;
  n -= (uint32_t)hn;
  if (n < 6) return false;
  uint32_t magic;
  memcpy(&magic, p, 4);
  uint32_t fhd = p[4];
  if (magic != kZstdMagic || (fhd & (dict ? 0x0c : 0x0f))) return false;
  uint32_t fcs = fhd >> 6, single = (fhd >> 5) & 1;
  uint32_t ip = 5 + !single + (fcs == 0 ? single : fcs == 1 ? 2 : fcs == 2 ? 4 : 8) +
                zstd_did_bytes(fhd);
  for (;;) {
    if (ip + 3 > n) return false;
    uint32_t h = p[ip] | (p[ip + 1] << 8) | ((uint32_t)p[ip + 2] << 16);
    uint32_t type = (h >> 1) & 3;
    if (type == 3) return false;
    ip += 3 + (type == 1 ? 1 : h >> 3);
    if (ip > n) return false;
    if (h & 1) return ip == n;
  }
}

#ifdef DCW_ZSTD_WAVE
// ---------------------------------------------------------------- wave form
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
#define ZFN __device__ inline
#define ZW_LANES for (uint32_t lane = zlane, zonce = 1; zonce; zonce = 0)
#define ZW_SYNC()                                        \
  do {                                                   \
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); \
    __builtin_amdgcn_s_waitcnt(0);                       \
    __builtin_amdgcn_wave_barrier();                     \
  } while (0)
#else
#define ZFN static inline
static int zw_descending = 0; // the host runs every frame in both lane orders
#define ZW_LANES \
  for (uint32_t zi = 0, lane = zw_descending ? 63 : 0; zi < 64; \
       zi++, lane = zw_descending ? 63 - zi : zi)
#define ZW_SYNC() ((void)0)
#endif

#ifdef DCW_ZSTD_STATS
enum ZStat {
  ZS_BLK_RAW, ZS_BLK_RLE, ZS_BLK_COMP,
  ZS_LIT_RAW, ZS_LIT_RLE, ZS_LIT_HUF1, ZS_LIT_HUF4, ZS_LIT_TREELESS,
  ZS_W_DIRECT, ZS_W_FSE,
  ZS_LL_PRE, ZS_LL_RLE, ZS_LL_FSE, ZS_LL_REP,
  ZS_OF_PRE, ZS_OF_RLE, ZS_OF_FSE, ZS_OF_REP,
  ZS_ML_PRE, ZS_ML_RLE, ZS_ML_FSE, ZS_ML_REP,
  ZS_REP1_LL0, ZS_REP2_LL0, ZS_REP3_LL0, ZS_REP1, ZS_REP2, ZS_REP3,
  ZS_NSEQ_0, ZS_NSEQ_1B, ZS_NSEQ_2B, ZS_NSEQ_3B, ZS_OVERLAP, ZS_COUNT
};
static uint32_t zstat[ZS_COUNT];
#define ZSTAT(i) (zstat[i]++)
#else
#define ZSTAT(i) ((void)0)
#endif

// FSE decode cell: next-state base | state bits << 16 | value bits << 24 |
// value base << 32 (the value is a literal length, a match length, an
// offset value or, for the Huffman weights' table, the weight itself)
enum { ZT_LL = 0, ZT_OF = 1, ZT_ML = 2, ZT_W = 3 };

struct alignas(16) ZstdWave {
  uint8_t in[kZstdMax + kZstdPad];  // the frame
  uint8_t out[kZstdMax + kZstdPad]; // the decoded block, all frame blocks
  uint8_t lit[kZstdMax + kZstdPad]; // Huffman/RLE literals (raw: in place);
                                    // scratch of the Huffman table build
  uint64_t tLL[512], tML[512], tOF[256], tW[64];
  uint64_t scan[64];
  uint16_t huf[2048]; // symbol | bits << 8
  uint32_t seq_ll[64], seq_ml[64], seq_off[64], seq_lp[64], seq_op[64];
  uint8_t fsym[512]; // spread symbols of the table being built
  int16_t norm[64];
  uint16_t cum[66];
  uint16_t rank[12], rstart[12], sbase[12];
  uint32_t hs_start[4], hs_len[4], hs_out[4], hs_cnt[4];
  uint32_t tlog[3]; // accuracy logs of tLL, tOF, tML as built
  uint32_t tpre[3]; // the table holds the predefined distribution
  uint32_t fail, ip, op, last, btype, bsize, bend;
  uint32_t have_huf, have_fse, rep1, rep2, rep3;
  uint32_t lit_size, lit_off, lit_inplace, lit_rle, lit_fill, lit_tree, litpos;
  uint32_t nstreams, hlog, hnsym, hnz, need_wfse, ws_start, ws_len, hs_rs, hs_rl;
  uint32_t nsym, blog, build, high;
  uint32_t nseq, modes, sq_start, stLL, stOF, stML;
  int32_t sq_pos;
};

// Where the frame, the decoded bytes and the literals live is a memory
// policy M beside the state ZS; the format code below is shared.  ZMemLds:
// all three are arrays of the ZstdWave.  (dcw_zstd_dec_large.h has the
// policy that keeps them in global memory.)  A policy comes with
//   zm_in(S, m)            the frame
//   zm_wscr(S)             1536 bytes of scratch for the Huffman table build
//   zm_huf_literals        the 1 or 4 Huffman streams -> literals
//   zm_rle_literals        RLE literals
//   zm_exec_batch          literal runs and matches of a placed batch
//   zm_tail_literals       the literals behind the last sequence
//   zm_plain_block         a raw or RLE block
// A policy may carry a preset dictionary too (dcw_zstd_dict.h).  The hooks for
// that have the defaults below, "no dictionary", which fold away:
//   zm_has_dict(m)         a Dictionary_ID field may stand in the frame header
//   zm_dict_id(m)          what a nonzero one must equal
//   zm_prefix_len(m)       bytes of dictionary content before output byte 0
//   zm_frame_begin         the dictionary's tables into S, behind the header
//   zm_dict_part           the part of a match that lies in the dictionary
struct ZMemLds {};
ZFN const uint8_t* zm_in(const ZstdWave& S, const ZMemLds&) { return S.in; }
template <class M> ZFN constexpr bool zm_has_dict(const M&) { return false; }
template <class M> ZFN constexpr uint32_t zm_dict_id(const M&) { return 0; }
template <class M> ZFN constexpr uint32_t zm_prefix_len(const M&) { return 0; }
template <class ZS, class M> ZFN void zm_frame_begin(ZS&, const M&, uint32_t) {}
template <class M>
ZFN constexpr uint32_t zm_dict_part(const M&, uint8_t*, uint32_t, uint32_t, uint32_t,
                                    uint32_t) { return 0; }
ZFN uint8_t* zm_wscr(ZstdWave& S) { return S.lit; }

ZFN uint32_t z_highbit(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }
ZFN uint64_t z_ld64(const uint8_t* p) {
  uint32_t lo, hi;
  memcpy(&lo, p, 4);
  memcpy(&hi, p + 4, 4);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// exclusive prefix sums of scan[0..64), in place
template <class ZS>
ZFN void zw_scan(ZS& S, uint32_t zlane) {
#if defined(__HIPCC__)
  ZW_SYNC();
  unsigned long long v = S.scan[zlane], inc = v;
  for (uint32_t sh = 1; sh < 64; sh <<= 1) {
    unsigned long long up = __shfl_up(inc, sh);
    if (zlane >= sh) inc += up;
  }
  S.scan[zlane] = inc - v;
  ZW_SYNC();
#else
  (void)zlane;
  uint64_t acc = 0;
  for (uint32_t i = 0; i < 64; i++) {
    uint64_t v = S.scan[i];
    S.scan[i] = acc;
    acc += v;
  }
#endif
}

// ---- backward bitstream: `pos` bits are left above the stream's start
struct ZBack {
  const uint8_t* p;
  int32_t pos;
};
ZFN bool zb_init(ZBack& b, const uint8_t* p, uint32_t len) {
  if (len == 0 || p[len - 1] == 0) return false;
  b.p = p;
  b.pos = (int32_t)(8 * (len - 1) + z_highbit(p[len - 1]));
  return true;
}
// the next nb (<= 32) bits; bits below the stream's start read as 0.  The
// 8-byte fetch may reach 7 bytes past the stream: inside kZstdPad.
ZFN uint32_t zb_peek(const ZBack& b, uint32_t nb) {
  if (nb == 0 || b.pos <= 0) return 0;
  if ((uint32_t)b.pos >= nb) {
    uint32_t lo = (uint32_t)b.pos - nb;
    return (uint32_t)((z_ld64(b.p + (lo >> 3)) >> (lo & 7)) & ((1ull << nb) - 1));
  }
  uint64_t w = z_ld64(b.p) & ((1ull << b.pos) - 1);
  return (uint32_t)(w << (nb - (uint32_t)b.pos));
}
ZFN uint32_t zb_read(ZBack& b, uint32_t nb) { // caller refuses on pos < 0
  uint32_t v = zb_peek(b, nb);
  b.pos -= (int32_t)nb;
  return v;
}

// ---- code tables, as arithmetic (no constant arrays to index)
ZFN void z_ll_code(uint32_t c, uint32_t* base, uint32_t* bits) {
  if (c < 16) { *base = c; *bits = 0; }
  else if (c < 20) { *base = 16 + 2 * (c - 16); *bits = 1; }
  else if (c < 22) { *base = 24 + 4 * (c - 20); *bits = 2; }
  else if (c < 24) { *base = 32 + 8 * (c - 22); *bits = 3; }
  else if (c == 24) { *base = 48; *bits = 4; }
  else { *bits = c - 19; *base = 1u << (c - 19); }
}
ZFN void z_ml_code(uint32_t c, uint32_t* base, uint32_t* bits) {
  if (c < 32) { *base = c + 3; *bits = 0; }
  else if (c < 36) { *base = 35 + 2 * (c - 32); *bits = 1; }
  else if (c < 38) { *base = 43 + 4 * (c - 36); *bits = 2; }
  else if (c < 40) { *base = 51 + 8 * (c - 38); *bits = 3; }
  else if (c < 42) { *base = 67 + 16 * (c - 40); *bits = 4; }
  else if (c == 42) { *base = 99; *bits = 5; }
  else { *bits = c - 36; *base = (1u << (c - 36)) + 3; }
}
ZFN uint64_t z_cell(uint32_t kind, uint32_t sym, uint32_t nb, uint32_t next) {
  uint32_t base = sym, bits = 0;
  if (kind == ZT_LL) z_ll_code(sym, &base, &bits);
  else if (kind == ZT_ML) z_ml_code(sym, &base, &bits);
  else if (kind == ZT_OF) { base = 1u << sym; bits = sym; }
  return (uint64_t)next | ((uint64_t)nb << 16) | ((uint64_t)bits << 24) |
         ((uint64_t)base << 32);
}
#define ZC_NEXT(e) ((uint32_t)(e) & 0xffffu)
#define ZC_NB(e) ((uint32_t)((e) >> 16) & 0xffu)
#define ZC_BITS(e) ((uint32_t)((e) >> 24) & 0xffu)
#define ZC_BASE(e) ((uint32_t)((e) >> 32))

// predefined distributions (RFC 8878 3.1.1.3.2.2)
ZFN int z_predef(uint32_t kind, uint32_t i) {
  if (kind == ZT_LL)
    return i == 0 ? 4 : i == 1 ? 3 : i < 13 ? 2 : i < 16 ? 1 : i < 25 ? 2
         : i == 25 ? 3 : i == 26 ? 2 : i < 32 ? 1 : -1;
  if (kind == ZT_ML)
    return i == 0 ? 1 : i == 1 ? 4 : i == 2 ? 3 : i < 9 ? 2 : i < 46 ? 1 : -1;
  return i < 6 ? 1 : i < 9 ? 2 : i < 24 ? 1 : -1;
}

// ---- FSE table description (forward bits, least significant first).  Bits
// past p[n) read as 0 and are refused at the end.  -> bytes used, 0: refuse
ZFN uint32_t zf_peek(const uint8_t* p, uint32_t n, uint32_t bit, uint32_t nb) {
  uint32_t byte = bit >> 3, v = 0;
  for (uint32_t k = 0; k < 4; k++)
    if (byte + k < n) v |= (uint32_t)p[byte + k] << (8 * k);
  return (v >> (bit & 7)) & ((1u << nb) - 1);
}
template <class ZS>
ZFN uint32_t zstd_read_ncount(ZS& S, const uint8_t* p, uint32_t n,
                              uint32_t max_sym, uint32_t max_log) {
  if (n == 0) return 0;
  uint32_t log = zf_peek(p, n, 0, 4) + 5, bit = 4;
  if (log > max_log) return 0;
  int remaining = (1 << log) + 1, threshold = 1 << log;
  uint32_t nbits = log + 1, sym = 0;
  bool prev0 = false;
  while (remaining > 1 && sym <= max_sym) {
    if (prev0) {
      uint32_t n0 = sym;
      for (;;) {
        uint32_t r = zf_peek(p, n, bit, 2);
        bit += 2;
        n0 += r;
        if (r != 3) break;
        if (n0 > max_sym) return 0;
      }
      if (n0 > max_sym) return 0;
      while (sym < n0) S.norm[sym++] = 0;
    }
    int max = 2 * threshold - 1 - remaining;
    int v = (int)zf_peek(p, n, bit, nbits), count;
    if ((v & (threshold - 1)) < max) {
      count = v & (threshold - 1);
      bit += nbits - 1;
    } else {
      count = v & (2 * threshold - 1);
      if (count >= threshold) count -= max;
      bit += nbits;
    }
    count--;
    remaining -= count < 0 ? -count : count;
    S.norm[sym++] = (int16_t)count;
    prev0 = count == 0;
    while (remaining < threshold) {
      nbits--;
      threshold >>= 1;
    }
  }
  if (remaining != 1 || bit > 8 * n) return 0;
  S.nsym = sym;
  S.blog = log;
  return (bit + 7) >> 3;
}

// ---- FSE decode table from norm[0..nsym) and blog, by the whole wave
template <class ZS>
ZFN void zstd_fse_build(ZS& S, uint64_t* T, uint32_t kind, uint32_t zlane) {
  const uint32_t log = S.blog, size = 1u << log, mask = size - 1;
  const uint32_t step = (size >> 1) + (size >> 3) + 3, nsym = S.nsym;
  const uint32_t per = (size + 63) >> 6;
  ZW_LANES {
    if (lane != 0) continue;
    uint32_t c = 0, hi = size - 1;
    for (uint32_t s = 0; s < nsym; s++) {
      S.cum[s] = (uint16_t)c;
      if (S.norm[s] > 0) c += (uint32_t)S.norm[s];
      else if (S.norm[s] < 0) S.fsym[hi--] = (uint8_t)s; // "less than 1": top
    }
    S.cum[nsym] = (uint16_t)c;
    S.high = hi;
  }
  ZW_SYNC();
  const uint32_t high = S.high;
  ZW_LANES { // visit indices [lane*per, +per): how many land above `high`
    uint32_t cnt = 0;
    for (uint32_t j = lane * per; j < lane * per + per && j < size; j++)
      cnt += ((j * step) & mask) > high;
    S.scan[lane] = cnt;
  }
  zw_scan(S, zlane);
  ZW_LANES {
    uint32_t j0 = lane * per;
    if (j0 >= size) continue;
    uint32_t r = j0 - (uint32_t)S.scan[lane]; // rank among the placed cells
    uint32_t lo = 0, hi = nsym;
    while (hi - lo > 1) {
      uint32_t mid = (lo + hi) >> 1;
      if (S.cum[mid] <= r) lo = mid; else hi = mid;
    }
    for (uint32_t j = j0; j < j0 + per && j < size; j++) {
      uint32_t pos = (j * step) & mask;
      if (pos > high) continue;
      while (r >= S.cum[lo + 1]) lo++;
      S.fsym[pos] = (uint8_t)lo;
      r++;
    }
  }
  ZW_SYNC();
  ZW_LANES { // one lane per symbol numbers its cells in table order
    if (lane >= nsym || S.norm[lane] == 0) continue;
    uint32_t next = S.norm[lane] < 0 ? 1u : (uint32_t)S.norm[lane];
    uint32_t left = next;
    for (uint32_t p = 0; p < size && left; p++) {
      if (S.fsym[p] != lane) continue;
      uint32_t nb = log - z_highbit(next);
      T[p] = z_cell(kind, lane, nb, (next << nb) - size);
      next++;
      left--;
    }
  }
  ZW_SYNC();
}

// ---- Huffman: weights -> rank layout (lane 0), then the table (wave)
template <class ZS>
ZFN void zstd_huf_weights_done(ZS& S, uint32_t nw) {
  uint8_t* W = zm_wscr(S);
  uint32_t total = 0;
  for (uint32_t w = 0; w < 12; w++) S.rank[w] = 0;
  for (uint32_t i = 0; i < nw; i++) {
    uint32_t w = W[i];
    if (w > 11) { S.fail = 1; return; }
    S.rank[w]++;
    total += (1u << w) >> 1;
  }
  if (total == 0) { S.fail = 1; return; }
  uint32_t log = z_highbit(total) + 1;
  uint32_t rest = (1u << log) - total;
  if (log > 11 || (rest & (rest - 1))) { S.fail = 1; return; }
  uint32_t lastw = z_highbit(rest) + 1;
  W[nw] = (uint8_t)lastw;
  S.rank[lastw]++;
  if (S.rank[1] < 2 || (S.rank[1] & 1)) { S.fail = 1; return; }
  uint32_t pos = 0, k = 0;
  for (uint32_t w = 1; w <= log; w++) {
    S.rstart[w] = (uint16_t)pos;
    S.sbase[w] = (uint16_t)k;
    pos += (uint32_t)S.rank[w] << (w - 1);
    k += S.rank[w];
  }
  S.hlog = log;
  S.hnsym = nw + 1;
  S.hnz = k;
}
template <class ZS>
ZFN void zstd_huf_build(ZS& S, uint32_t zlane) {
  (void)zlane;
  const uint32_t log = S.hlog, nsym = S.hnsym, nz = S.hnz, size = 1u << log;
  const uint8_t* W = zm_wscr(S);
  uint16_t* sstart = (uint16_t*)(zm_wscr(S) + 512);  // by table position:
  uint16_t* sval = (uint16_t*)(zm_wscr(S) + 1024);   // first cell, cell value
  ZW_LANES { // one lane per weight: its symbols in order, lowest cells first
    if (lane < 1 || lane > log) continue;
    uint32_t k = S.sbase[lane], cur = S.rstart[lane];
    for (uint32_t s = 0; s < nsym; s++) {
      if (W[s] != lane) continue;
      sstart[k] = (uint16_t)cur;
      sval[k] = (uint16_t)(s | ((log + 1 - lane) << 8));
      k++;
      cur += 1u << (lane - 1);
    }
  }
  ZW_SYNC();
  const uint32_t per = (size + 63) >> 6;
  ZW_LANES {
    uint32_t a = lane * per;
    if (a >= size) continue;
    uint32_t lo = 0, hi = nz;
    while (hi - lo > 1) {
      uint32_t mid = (lo + hi) >> 1;
      if (sstart[mid] <= a) lo = mid; else hi = mid;
    }
    for (uint32_t u = a; u < a + per && u < size; u++) {
      while (lo + 1 < nz && sstart[lo + 1] <= u) lo++;
      S.huf[u] = sval[lo];
    }
  }
  ZW_SYNC();
}
ZFN void zstd_huf_stream(ZstdWave& S, uint32_t k) {
  ZBack b;
  if (!zb_init(b, S.in + S.hs_start[k], S.hs_len[k])) { S.fail = 1; return; }
  uint8_t* o = S.lit + S.hs_out[k];
  const uint32_t cnt = S.hs_cnt[k], log = S.hlog;
  for (uint32_t i = 0; i < cnt; i++) {
    if (b.pos <= 0) { S.fail = 1; return; }
    uint32_t e = S.huf[zb_peek(b, log)];
    o[i] = (uint8_t)e;
    b.pos -= (int32_t)(e >> 8);
  }
  if (b.pos != 0) S.fail = 1;
}
// the Huffman weights' own FSE stream: two interleaved states (lane 0)
template <class ZS>
ZFN void zstd_huf_fse_weights(ZS& S, const uint8_t* in) {
  ZBack b;
  if (!zb_init(b, in + S.ws_start, S.ws_len)) { S.fail = 1; return; }
  uint8_t* W = zm_wscr(S);
  uint32_t s1 = zb_read(b, S.blog), s2 = zb_read(b, S.blog), n = 0;
  if (b.pos < 0) { S.fail = 1; return; }
  for (;;) {
    if (n > 253) { S.fail = 1; return; }
    uint64_t e = S.tW[s1];
    W[n++] = (uint8_t)ZC_BASE(e);
    if ((int32_t)ZC_NB(e) > b.pos) { W[n++] = (uint8_t)ZC_BASE(S.tW[s2]); break; }
    s1 = ZC_NEXT(e) + zb_read(b, ZC_NB(e));
    if (n > 253) { S.fail = 1; return; }
    e = S.tW[s2];
    W[n++] = (uint8_t)ZC_BASE(e);
    if ((int32_t)ZC_NB(e) > b.pos) { W[n++] = (uint8_t)ZC_BASE(S.tW[s1]); break; }
    s2 = ZC_NEXT(e) + zb_read(b, ZC_NB(e));
  }
  zstd_huf_weights_done(S, n);
}
// where the 1 or 4 streams lie (lane 0); region = [hs_rs, +hs_rl)
template <class ZS>
ZFN void zstd_lit_streams(ZS& S, const uint8_t* in) {
  uint32_t rs = S.hs_rs, rl = S.hs_rl, ls = S.lit_size;
  if (S.nstreams == 1) {
    S.hs_start[0] = rs; S.hs_len[0] = rl; S.hs_out[0] = 0; S.hs_cnt[0] = ls;
    return;
  }
  if (rl < 10) { S.fail = 1; return; }
  const uint8_t* p = in + rs;
  uint32_t l1 = p[0] | (p[1] << 8), l2 = p[2] | (p[3] << 8), l3 = p[4] | (p[5] << 8);
  uint32_t seg = (ls + 3) >> 2;
  if (6 + l1 + l2 + l3 > rl || 3 * seg > ls) { S.fail = 1; return; }
  uint32_t at = rs + 6;
  for (uint32_t k = 0; k < 4; k++) {
    uint32_t len = k == 0 ? l1 : k == 1 ? l2 : k == 2 ? l3 : rs + rl - at;
    S.hs_start[k] = at; S.hs_len[k] = len;
    S.hs_out[k] = k * seg; S.hs_cnt[k] = k < 3 ? seg : ls - 3 * seg;
    at += len;
  }
}

// ---- headers (lane 0)
template <class ZS, class M>
ZFN void zstd_frame_header(ZS& S, const M& m, const uint8_t* in, uint32_t n,
                           uint32_t cap) {
  S.fail = 0; S.op = 0; S.last = 0;
  S.have_huf = S.have_fse = 0;
  S.rep1 = 1; S.rep2 = 4; S.rep3 = 8;
  const uint8_t* p = in;
  if (n < 6) { S.fail = 1; return; }
  uint32_t magic;
  memcpy(&magic, p, 4);
  uint32_t fhd = p[4], fcs = fhd >> 6, single = (fhd >> 5) & 1;
  // content checksum, reserved bit: none of them here; a dictionary ID only
  // where the policy has a dictionary
  if (magic != kZstdMagic || (fhd & (zm_has_dict(m) ? 0x0c : 0x0f))) {
    S.fail = 1;
    return;
  }
  uint32_t ip = 5;
  if (!single) {
    if ((uint32_t)(p[ip] >> 3) + 10 > 31) { S.fail = 1; return; }
    ip++;
  }
  if (zm_has_dict(m) && (fhd & 3)) { // nonzero: the dictionary's, as libzstd
    uint32_t dl = zstd_did_bytes(fhd), id = 0;  // (ZSTD_decodeFrameHeader)
    if (ip + dl > n) { S.fail = 1; return; }
    for (uint32_t k = 0; k < dl; k++) id |= (uint32_t)p[ip + k] << (8 * k);
    if (id && id != zm_dict_id(m)) { S.fail = 1; return; }
    ip += dl;
  }
  uint32_t fb = fcs == 0 ? single : fcs == 1 ? 2 : fcs == 2 ? 4 : 8;
  if (ip + fb > n) { S.fail = 1; return; }
  if (fb) {
    uint64_t v = 0;
    for (uint32_t k = 0; k < fb; k++) v |= (uint64_t)p[ip + k] << (8 * k);
    if (fb == 2) v += 256;
    if (v != cap) { S.fail = 1; return; }
  }
  S.ip = ip + fb;
}
template <class ZS>
ZFN void zstd_block_header(ZS& S, const uint8_t* in, uint32_t n, uint32_t cap) {
  uint32_t ip = S.ip;
  if (ip + 3 > n) { S.fail = 1; return; }
  const uint8_t* p = in + ip;
  uint32_t h = p[0] | (p[1] << 8) | ((uint32_t)p[2] << 16);
  uint32_t type = (h >> 1) & 3, sz = h >> 3;
  ip += 3;
  S.last = h & 1; S.btype = type; S.bsize = sz;
  uint32_t stored = type == 1 ? 1 : sz;
  // a compressed block of Block_Maximum_Size is refused as by libzstd
  if (type == 3 || stored > n - ip || (type == 2 && sz < 3) ||
      (type != 2 && sz > cap - S.op) || sz > kZstdBlockMax ||
      (type == 2 && sz == kZstdBlockMax)) { S.fail = 1; return; }
  S.ip = ip;
  S.bend = ip + stored;
}
// A Huffman tree description at in[at], of at most lim bytes (lane 0): the
// weights, or for FSE-compressed weights need_wfse and where their stream
// lies.  -> its size, 0: refuse
template <class ZS>
ZFN uint32_t zstd_huf_tree_desc(ZS& S, const uint8_t* in, uint32_t at, uint32_t lim) {
  if (lim == 0) return 0;
  uint32_t hb = in[at], desc;
  uint8_t* W = zm_wscr(S);
  if (hb >= 128) { // direct 4-bit weights
    ZSTAT(ZS_W_DIRECT);
    uint32_t nw = hb - 127;
    desc = 1 + ((nw + 1) >> 1);
    if (desc > lim) return 0;
    for (uint32_t i = 0; i < nw; i++) {
      uint32_t b = in[at + 1 + (i >> 1)];
      W[i] = (uint8_t)((i & 1) ? (b & 15) : (b >> 4));
    }
    zstd_huf_weights_done(S, nw);
  } else { // FSE-compressed weights: description now, stream after the build
    ZSTAT(ZS_W_FSE);
    desc = 1 + hb;
    if (hb == 0 || desc > lim) return 0;
    uint32_t c = zstd_read_ncount(S, in + at + 1, hb, 11, 6);
    if (c == 0 || c >= hb) return 0;
    S.need_wfse = 1;
    S.ws_start = at + 1 + c;
    S.ws_len = hb - c;
  }
  return S.fail ? 0 : desc;
}
template <class ZS>
ZFN void zstd_lit_header(ZS& S, const uint8_t* in, uint32_t cap) {
  const uint32_t bs = S.ip, bsz = S.bend - bs; // bsz >= 3
  const uint8_t* p = in + bs;
  uint32_t type = p[0] & 3, sf = (p[0] >> 2) & 3, lh, ls, cs = 0;
  S.lit_inplace = S.lit_fill = S.need_wfse = 0;
  S.lit_tree = type == 2;
  S.nstreams = 0;
  S.litpos = 0;
  if (type < 2) {
    if (!(sf & 1)) { lh = 1; ls = p[0] >> 3; }
    else if (sf == 1) { lh = 2; ls = (p[0] | (p[1] << 8)) >> 4; }
    else { lh = 3; ls = (p[0] | (p[1] << 8) | ((uint32_t)p[2] << 16)) >> 4; }
    if (ls > cap - S.op || ls > kZstdBlockMax || lh + (type == 0 ? ls : 1) > bsz) {
      S.fail = 1;
      return;
    }
    S.lit_size = ls;
    if (type == 0) {
      ZSTAT(ZS_LIT_RAW);
      S.lit_inplace = 1;
      S.lit_off = bs + lh;
      S.ip = bs + lh + ls;
    } else {
      ZSTAT(ZS_LIT_RLE);
      S.lit_fill = 1;
      S.lit_rle = p[lh];
      S.ip = bs + lh + 1;
    }
    return;
  }
  if (bsz < 5) { S.fail = 1; return; }
  uint32_t lhc = p[0] | (p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  if (sf < 2) { lh = 3; ls = (lhc >> 4) & 0x3ff; cs = (lhc >> 14) & 0x3ff; }
  else if (sf == 2) { lh = 4; ls = (lhc >> 4) & 0x3fff; cs = lhc >> 18; }
  else { lh = 5; ls = (lhc >> 4) & 0x3ffff; cs = (lhc >> 22) + ((uint32_t)p[4] << 10); }
  S.nstreams = sf == 0 ? 1 : 4;
  if (ls == 0 || cs == 0 || ls > cap - S.op || ls > kZstdBlockMax || lh + cs > bsz ||
      (type == 3 && !S.have_huf)) { S.fail = 1; return; }
  S.lit_size = ls;
  S.ip = bs + lh + cs;
  ZSTAT(sf == 0 ? ZS_LIT_HUF1 : ZS_LIT_HUF4);
  uint32_t at = bs + lh; // tree description, then the streams
  if (type == 3) {
    ZSTAT(ZS_LIT_TREELESS);
    S.hs_rs = at; S.hs_rl = cs;
    zstd_lit_streams(S, in);
    return;
  }
  S.have_huf = 1;
  const uint32_t desc = zstd_huf_tree_desc(S, in, at, cs - 1);
  if (desc == 0) { S.fail = 1; return; }
  S.hs_rs = at + desc; S.hs_rl = cs - desc;
  zstd_lit_streams(S, in);
}
template <class ZS>
ZFN void zstd_seq_header(ZS& S, const uint8_t* in) {
  uint32_t ip = S.ip, bend = S.bend;
  S.nseq = 0;
  if (ip >= bend) { S.fail = 1; return; }
  uint32_t b0 = in[ip++], nseq;
  if (b0 == 0) {
    ZSTAT(ZS_NSEQ_0);
    if (ip != bend) S.fail = 1;
    return;
  }
  if (b0 < 128) { nseq = b0; ZSTAT(ZS_NSEQ_1B); }
  else if (b0 < 255) {
    if (ip >= bend) { S.fail = 1; return; }
    nseq = ((b0 - 128) << 8) + in[ip++];
    if (nseq == 0) { S.fail = 1; return; }
    ZSTAT(ZS_NSEQ_2B);
  } else {
    if (ip + 2 > bend) { S.fail = 1; return; }
    nseq = (in[ip] | (in[ip + 1] << 8)) + 0x7f00;
    ip += 2;
    ZSTAT(ZS_NSEQ_3B);
  }
  if (ip >= bend) { S.fail = 1; return; }
  S.modes = in[ip++];
  if (S.modes & 3) { S.fail = 1; return; }
  S.nseq = nseq;
  S.ip = ip;
}
// table t of the block (0 LL, 1 OF, 2 ML): read its mode's description
template <class ZS>
ZFN void zstd_seq_table(ZS& S, const uint8_t* in, uint32_t t) {
  const uint32_t mode = (S.modes >> (6 - 2 * t)) & 3;
  const uint32_t max_sym = t == ZT_LL ? 35 : t == ZT_OF ? 31 : 52;
  uint64_t* T = t == ZT_LL ? S.tLL : t == ZT_OF ? S.tOF : S.tML;
  S.build = 0;
  if (mode == 0) {
    ZSTAT(ZS_LL_PRE + 4 * t);
    if (S.tpre[t]) return;
    S.nsym = max_sym == 31 ? 29 : max_sym + 1;
    S.blog = t == ZT_OF ? 5 : 6;
    for (uint32_t i = 0; i < S.nsym; i++) S.norm[i] = (int16_t)z_predef(t, i);
    S.build = 1;
    S.tpre[t] = 1;
  } else if (mode == 1) {
    ZSTAT(ZS_LL_RLE + 4 * t);
    if (S.ip >= S.bend || in[S.ip] > max_sym) { S.fail = 1; return; }
    T[0] = z_cell(t, in[S.ip++], 0, 0);
    S.tlog[t] = 0;
    S.tpre[t] = 0;
  } else if (mode == 2) {
    ZSTAT(ZS_LL_FSE + 4 * t);
    uint32_t c = zstd_read_ncount(S, in + S.ip, S.bend - S.ip, max_sym,
                                  t == ZT_OF ? 8 : 9);
    if (c == 0) { S.fail = 1; return; }
    S.ip += c;
    S.build = 1;
    S.tpre[t] = 0;
  } else {
    ZSTAT(ZS_LL_REP + 4 * t);
    if (!S.have_fse) S.fail = 1;
  }
  if (S.build) S.tlog[t] = S.blog;
}
template <class ZS>
ZFN void zstd_seq_init(ZS& S, const uint8_t* in) {
  ZBack b;
  if (!zb_init(b, in + S.ip, S.bend - S.ip)) { S.fail = 1; return; }
  S.stLL = zb_read(b, S.tlog[ZT_LL]);
  S.stOF = zb_read(b, S.tlog[ZT_OF]);
  S.stML = zb_read(b, S.tlog[ZT_ML]);
  if (b.pos < 0) { S.fail = 1; return; }
  S.sq_start = S.ip;
  S.sq_pos = b.pos;
  S.have_fse = 1;
}
// lane 0: the next cnt (<= 64) sequences into seq_ll/seq_ml/seq_off
template <class ZS>
ZFN void zstd_seq_batch(ZS& S, const uint8_t* in, uint32_t cnt, bool final_batch) {
  ZBack b = {in + S.sq_start, S.sq_pos};
  uint32_t sl = S.stLL, so = S.stOF, sm = S.stML;
  uint32_t r1 = S.rep1, r2 = S.rep2, r3 = S.rep3;
  for (uint32_t k = 0; k < cnt; k++) {
    uint64_t el = S.tLL[sl], eo = S.tOF[so], em = S.tML[sm];
    uint32_t ofv = ZC_BASE(eo) + zb_read(b, ZC_BITS(eo));
    uint32_t ml = ZC_BASE(em) + zb_read(b, ZC_BITS(em));
    uint32_t ll = ZC_BASE(el) + zb_read(b, ZC_BITS(el));
    if (b.pos < 0) { S.fail = 1; return; }
    uint32_t off;
    if (ofv > 3) {
      off = ofv - 3;
      r3 = r2; r2 = r1; r1 = off;
    } else {
      uint32_t idx = ofv - 1 + (ll == 0);
      ZSTAT((ll == 0 ? ZS_REP1_LL0 : ZS_REP1) + ofv - 1);
      if (idx == 0) off = r1;
      else if (idx == 1) { off = r2; r2 = r1; r1 = off; }
      else {
        off = idx == 2 ? r3 : r1 - 1;
        if (off == 0) { S.fail = 1; return; }
        r3 = r2; r2 = r1; r1 = off;
      }
    }
    S.seq_ll[k] = ll; S.seq_ml[k] = ml; S.seq_off[k] = off;
    if (off < ml) ZSTAT(ZS_OVERLAP);
    if (final_batch && k + 1 == cnt) break;
    sl = ZC_NEXT(el) + zb_read(b, ZC_NB(el));
    sm = ZC_NEXT(em) + zb_read(b, ZC_NB(em));
    so = ZC_NEXT(eo) + zb_read(b, ZC_NB(eo));
    if (b.pos < 0) { S.fail = 1; return; }
  }
  if (final_batch && b.pos != 0) { S.fail = 1; return; }
  S.sq_pos = b.pos;
  S.stLL = sl; S.stOF = so; S.stML = sm;
  S.rep1 = r1; S.rep2 = r2; S.rep3 = r3;
}

// ---- ZMemLds: the moves of a block inside the ZstdWave
ZFN bool zm_huf_literals(ZstdWave& S, const ZMemLds&, uint32_t zlane) {
  (void)zlane;
  const uint32_t ns = S.nstreams;
  ZW_LANES { if (lane < ns) zstd_huf_stream(S, lane); }
  ZW_SYNC();
  return !S.fail;
}
ZFN void zm_rle_literals(ZstdWave& S, const ZMemLds&, uint32_t zlane) {
  (void)zlane;
  const uint32_t ls = S.lit_size, v = S.lit_rle;
  ZW_LANES { for (uint32_t i = lane; i < ls; i += 64) S.lit[i] = (uint8_t)v; }
  ZW_SYNC();
}
template <class M>
ZFN void zm_exec_batch(ZstdWave& S, const M& m, uint32_t cnt, uint32_t zlane) {
  (void)zlane;
  const uint8_t* lit = S.lit_inplace ? S.in + S.lit_off : S.lit;
  ZW_LANES { // all literal runs of the batch, one per lane
    if (lane >= cnt) continue;
    const uint8_t* s = lit + S.seq_lp[lane];
    uint8_t* d = S.out + S.seq_op[lane];
    for (uint32_t i = 0, ll = S.seq_ll[lane]; i < ll; i++) d[i] = s[i];
  }
  ZW_SYNC();
  for (uint32_t k = 0; k < cnt; k++) { // matches in order, the wave on each
    uint32_t ml = S.seq_ml[k];
    const uint32_t off = S.seq_off[k], at = S.seq_op[k] + S.seq_ll[k];
    uint8_t* d = S.out + at;
    const uint32_t pre = zm_dict_part(m, d, at, off, ml, zlane);
    d += pre;
    ml -= pre;
    const uint8_t* s = d - off;
    ZW_LANES {
      if (off >= ml) {
        for (uint32_t i = lane; i < ml; i += 64) d[i] = s[i];
      } else { // the period's bytes lie wholly below d: s[i % off]
        uint32_t r = lane % off, st = 64 % off;
        for (uint32_t i = lane; i < ml; i += 64) {
          d[i] = s[r];
          r += st;
          if (r >= off) r -= off;
        }
      }
    }
    ZW_SYNC();
  }
}
ZFN void zm_tail_literals(ZstdWave& S, const ZMemLds&, uint32_t rem, uint32_t op,
                          uint32_t zlane) {
  (void)zlane;
  const uint8_t* s = (S.lit_inplace ? S.in + S.lit_off : S.lit) + S.litpos;
  ZW_LANES { for (uint32_t i = lane; i < rem; i += 64) S.out[op + i] = s[i]; }
  ZW_SYNC();
}
ZFN void zm_plain_block(ZstdWave& S, const ZMemLds&, uint32_t type, uint32_t ip,
                        uint32_t op, uint32_t sz, uint32_t zlane) {
  (void)zlane;
  ZW_LANES {
    for (uint32_t i = lane; i < sz; i += 64)
      S.out[op + i] = S.in[type == 0 ? ip + i : ip];
  }
  ZW_SYNC();
}

// ---- one compressed block; false: refused
template <class ZS, class M>
ZFN bool zstd_block(ZS& S, const M& m, uint32_t cap, uint32_t zlane) {
  const uint8_t* in = zm_in(S, m);
  ZW_LANES { if (lane == 0) zstd_lit_header(S, in, cap); }
  ZW_SYNC();
  if (S.fail) return false;
  if (S.need_wfse) {
    zstd_fse_build(S, S.tW, ZT_W, zlane);
    ZW_LANES { if (lane == 0) zstd_huf_fse_weights(S, in); }
    ZW_SYNC();
    if (S.fail) return false;
  }
  if (S.nstreams) {
    // a new tree's table; a treeless block decodes with the table in place
    if (S.lit_tree) zstd_huf_build(S, zlane);
    if (!zm_huf_literals(S, m, zlane)) return false;
  } else if (S.lit_fill) {
    zm_rle_literals(S, m, zlane);
  }
  ZW_LANES { if (lane == 0) zstd_seq_header(S, in); }
  ZW_SYNC();
  if (S.fail) return false;
  if (S.nseq) {
    for (uint32_t t = 0; t < 3; t++) {
      ZW_LANES { if (lane == 0) zstd_seq_table(S, in, t); }
      ZW_SYNC();
      if (S.fail) return false;
      if (S.build)
        zstd_fse_build(S, t == ZT_LL ? S.tLL : t == ZT_OF ? S.tOF : S.tML, t, zlane);
    }
    ZW_LANES { if (lane == 0) zstd_seq_init(S, in); }
    ZW_SYNC();
    if (S.fail) return false;
  }
  for (uint32_t left = S.nseq; left;) {
    const uint32_t cnt = left < 64 ? left : 64;
    left -= cnt;
    ZW_LANES { if (lane == 0) zstd_seq_batch(S, in, cnt, left == 0); }
    ZW_SYNC();
    if (S.fail) return false;
    ZW_LANES {
      uint64_t ll = lane < cnt ? S.seq_ll[lane] : 0, ml = lane < cnt ? S.seq_ml[lane] : 0;
      S.scan[lane] = ll | ((ll + ml) << 32);
    }
    zw_scan(S, zlane);
    ZW_LANES { // positions of run and match; every bound before any move
      if (lane >= cnt) continue;
      uint32_t ll = S.seq_ll[lane], ml = S.seq_ml[lane];
      uint32_t lp = S.litpos + (uint32_t)S.scan[lane];
      uint32_t o = S.op + (uint32_t)(S.scan[lane] >> 32);
      if (lp > S.lit_size || ll > S.lit_size - lp || o > cap || ll + ml > cap - o ||
          S.seq_off[lane] > o + ll + zm_prefix_len(m))
        S.fail = 1;
      S.seq_lp[lane] = lp;
      S.seq_op[lane] = o;
    }
    ZW_SYNC();
    if (S.fail) return false;
    zm_exec_batch(S, m, cnt, zlane);
    ZW_LANES {
      if (lane != cnt - 1) continue;
      S.litpos = S.seq_lp[lane] + S.seq_ll[lane];
      S.op = S.seq_op[lane] + S.seq_ll[lane] + S.seq_ml[lane];
    }
    ZW_SYNC();
  }
  const uint32_t rem = S.lit_size - S.litpos, op = S.op;
  if (rem > cap - op) return false;
  zm_tail_literals(S, m, rem, op, zlane);
  ZW_LANES { if (lane == 0) { S.op = op + rem; S.ip = S.bend; } }
  ZW_SYNC();
  return true;
}

// The frame of n bytes -> cap decoded bytes, both where the policy has them.
// Uniform result: every lane returns the same.
template <class ZS, class M>
ZFN bool zstd_dec_frame(ZS& S, const M& m, uint32_t n, uint32_t cap, uint32_t zlane) {
  const uint8_t* in = zm_in(S, m);
  ZW_LANES { if (lane == 0) zstd_frame_header(S, m, in, n, cap); }
  ZW_SYNC();
  if (S.fail) return false;
  zm_frame_begin(S, m, zlane);
  for (;;) {
    ZW_LANES { if (lane == 0) zstd_block_header(S, in, n, cap); }
    ZW_SYNC();
    if (S.fail) return false;
    const uint32_t type = S.btype, sz = S.bsize, ip = S.ip, op = S.op;
    if (type == 2) {
      ZSTAT(ZS_BLK_COMP);
      if (!zstd_block(S, m, cap, zlane)) return false;
    } else {
      ZSTAT(type == 0 ? ZS_BLK_RAW : ZS_BLK_RLE);
      zm_plain_block(S, m, type, ip, op, sz, zlane);
      ZW_LANES { if (lane == 0) { S.op = op + sz; S.ip = S.bend; } }
      ZW_SYNC();
    }
    if (S.last) break;
  }
  return S.ip == n && S.op == cap;
}
// The frame in S.in[0, n) -> S.out[0, cap).  n, cap <= kZstdMax.
ZFN bool zstd_dec_wave(ZstdWave& S, uint32_t n, uint32_t cap, uint32_t zlane) {
  return zstd_dec_frame(S, ZMemLds(), n, cap, zlane);
}
#endif // DCW_ZSTD_WAVE

} // namespace dcw
