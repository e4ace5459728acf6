// dcw_zstd_dec_large.h — the zstd frame decoder of dcw_zstd_dec.h for frames
// that its LDS staging cannot hold: stored or decoded size over kZstdMax.
// Included by dcw_k_decode.h for the GPU (k_decompress_zstd_large), by
// dcw_worker.cpp for the eligibility walk and by tools/zstd_large_host.
//
// The format code (headers, table builds, sequence batches, repeat offsets)
// is dcw_zstd_dec.h's, shared through its memory policy.  Here the policy is
// ZMemGlobal: the frame stays where it was staged, the decoded bytes go
// straight to the block's slot of the decoded blob, and Huffman literals go
// to a scratch area in global memory that the work-group owns.  LDS
// (ZstdLargeLds) holds tables and batch state only.
//
// Every move is a move of the whole wave:
//   Huffman literals  lanes 0..3 decode their streams kZRingPart symbols at a
//                     time into their parts of `ring`; the wave then flushes
//                     the parts with one 16-byte store per lane
//   literal runs      all runs of a batch are one contiguous stretch of the
//                     literals: lane i takes byte i, i + 64, ... of it and
//                     finds the run it falls in by bisection over seq_lp
//   matches           in sequence order, 64 bytes per step, or 1 KiB per
//                     step (16 bytes per lane) where source and destination
//                     do not overlap; raw blocks, RLE blocks and the
//                     trailing literals move the same way
// A match reads what the wave stored earlier, in this zstd block or in any
// block before it.  Between the store and the load lies a ZW_SYNC(): its
// fence and its wait for every outstanding store make the bytes visible to
// the other lanes of the wave, which share the compute unit's vector cache.
//
// Reads: the 8-byte fetches of the backward bitstreams may reach 7 bytes past
// a stream, so past the stored block.  Behind every stored block of the
// staged blob lie its 5-byte trailer and then either more of the file (an
// SST ends in a 53-byte footer) or, behind the last block of a rebuilt blob,
// the >= 64 bytes of slack of DevBuf::reserve: the fetch stays inside the
// staging buffer.  Nothing else reads past what it copies.
// Writes: only out[0, cap) and the work-group's own literal scratch.
#pragma once
#include "dcw_zstd_dec.h"

namespace dcw {

// The eligibility walk of the large decoder: zstd_eligible() without the two
// kZstdMax bounds.  One plain frame (no dictionary ID, no content checksum,
// reserved bit clear) whose block headers chain exactly to the end of the
// payload, no Block_Size over 128 KiB, promised size at most 0x7fffffff.
// Touches p[0, n) only.  `dict` as for zstd_eligible().
ZHD bool zstd_eligible_large(const uint8_t* p, uint32_t n, bool dict = false) {
  uint32_t un;
  int hn = zstd_preamble(p, n, &un);
  if (hn < 0 || un > 0x7fffffffu) return false;
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
    if (type == 3 || (h >> 3) > (128u << 10)) return false;
    ip += 3 + (type == 1 ? 1 : h >> 3);
    if (ip > n) return false;
    if (h & 1) return ip == n;
  }
}

// literal scratch of one work-group: a zstd block regenerates at most
// Block_Maximum_Size literals; the pad is a guard band between the areas of
// two work-groups that no move is meant to reach
static const uint32_t kZLitPad = 64;
static const uint32_t kZLitStride = (128u << 10) + kZLitPad;

#if defined(__HIPCC__)
// dcw_zstd_large.hip: k_decompress_zstd_large over `list`, one work-group of
// one wave per grid entry; litscr holds grid * kZLitStride bytes
void launch_decompress_zstd_large(uint32_t grid, hipStream_t stream,
                                  const uint8_t* blob, const uint64_t* boff,
                                  const uint32_t* bsize, const uint64_t* uoff,
                                  const uint32_t* usize, const uint32_t* list,
                                  uint32_t nlist, uint8_t* ublob, uint8_t* litscr,
                                  uint32_t* err_flag, uint32_t err_code);
#endif

#ifdef DCW_ZSTD_WAVE
static const uint32_t kZRingPart = 256; // x 4 streams = 64 lanes x 16 bytes

// ZstdWave without in/out/lit; `ring` and `wscr` instead
struct alignas(16) ZstdLargeLds {
  uint64_t tLL[512], tML[512], tOF[256], tW[64];
  uint64_t scan[64];
  uint8_t ring[4 * kZRingPart]; // Huffman symbols on their way to the scratch
  uint8_t wscr[1536];           // scratch of the Huffman table build
  uint16_t huf[2048];           // symbol | bits << 8
  uint32_t seq_ll[64], seq_ml[64], seq_off[64], seq_lp[64], seq_op[64];
  uint8_t fsym[512];
  int16_t norm[64];
  uint16_t cum[66];
  uint16_t rank[12], rstart[12], sbase[12];
  uint32_t hs_start[4], hs_len[4], hs_out[4], hs_cnt[4];
  int32_t hs_pos[4]; // bits left in each stream between two ring rounds
  uint32_t tlog[3];
  uint32_t tpre[3];
  uint32_t fail, ip, op, last, btype, bsize, bend;
  uint32_t have_huf, have_fse, rep1, rep2, rep3;
  uint32_t lit_size, lit_off, lit_inplace, lit_rle, lit_fill, lit_tree, litpos;
  uint32_t nstreams, hlog, hnsym, hnz, need_wfse, ws_start, ws_len, hs_rs, hs_rl;
  uint32_t nsym, blog, build, high;
  uint32_t nseq, modes, sq_start, stLL, stOF, stML;
  int32_t sq_pos;
};

struct ZMemGlobal {
  const uint8_t* in; // the frame, in the staged blob
  uint8_t* out;      // the block's slot in the decoded blob
  uint8_t* lit;      // kZLitStride bytes of scratch, 16-byte aligned
};
ZFN const uint8_t* zm_in(const ZstdLargeLds&, const ZMemGlobal& m) { return m.in; }
ZFN uint8_t* zm_wscr(ZstdLargeLds& S) { return S.wscr; }

// s[0, n) -> d[0, n) by the wave; the ranges must not overlap.  1 KiB per
// step, the last n % 16 bytes one per lane.
#define ZL_COPY(d, s, n)                                                  \
  ZW_LANES {                                                              \
    for (uint32_t t = lane * 16; t + 16 <= (n); t += 64 * 16) {           \
      uint64_t zv[2];                                                     \
      memcpy(zv, (s) + t, 16);                                            \
      memcpy((d) + t, zv, 16);                                            \
    }                                                                     \
    uint32_t t = ((n) & ~15u) + lane;                                     \
    if (lane < 16 && t < (n)) (d)[t] = (s)[t];                            \
  }
#define ZL_FILL(d, byte, n)                                               \
  ZW_LANES {                                                              \
    uint64_t zv[2];                                                       \
    zv[0] = zv[1] = 0x0101010101010101ull * (uint8_t)(byte);               \
    for (uint32_t t = lane * 16; t + 16 <= (n); t += 64 * 16)             \
      memcpy((d) + t, zv, 16);                                            \
    uint32_t t = ((n) & ~15u) + lane;                                     \
    if (lane < 16 && t < (n)) (d)[t] = (uint8_t)(byte);                   \
  }

// The 1 or 4 Huffman streams -> m.lit[0, lit_size).  A stream lane never
// stores to global memory: it fills its part of the ring, and the wave
// flushes the four parts, lane l the 16 bytes l % 16 of part l / 16.
ZFN bool zm_huf_literals(ZstdLargeLds& S, const ZMemGlobal& m, uint32_t zlane) {
  (void)zlane;
  const uint32_t ns = S.nstreams, log = S.hlog;
  ZW_LANES {
    if (lane >= ns) continue;
    ZBack b;
    if (!zb_init(b, m.in + S.hs_start[lane], S.hs_len[lane])) { S.fail = 1; continue; }
    S.hs_pos[lane] = b.pos;
  }
  ZW_SYNC();
  if (S.fail) return false;
  const uint32_t most = S.hs_cnt[0]; // no stream regenerates more than the first
  for (uint32_t base = 0; base < most; base += kZRingPart) {
    ZW_LANES {
      if (lane >= ns || base >= S.hs_cnt[lane]) continue;
      uint32_t cnt = S.hs_cnt[lane] - base;
      if (cnt > kZRingPart) cnt = kZRingPart;
      ZBack b = {m.in + S.hs_start[lane], S.hs_pos[lane]};
      uint8_t* o = S.ring + lane * kZRingPart;
      for (uint32_t i = 0; i < cnt; i++) {
        if (b.pos <= 0) { S.fail = 1; break; }
        uint32_t e = S.huf[zb_peek(b, log)];
        o[i] = (uint8_t)e;
        b.pos -= (int32_t)(e >> 8);
      }
      S.hs_pos[lane] = b.pos;
    }
    ZW_SYNC();
    if (S.fail) return false;
    ZW_LANES {
      const uint32_t k = lane >> 4, t = (lane & 15) * 16;
      if (k >= ns || base >= S.hs_cnt[k]) continue;
      uint32_t cnt = S.hs_cnt[k] - base;
      if (cnt > kZRingPart) cnt = kZRingPart;
      const uint8_t* s = S.ring + k * kZRingPart;
      uint8_t* d = m.lit + S.hs_out[k] + base;
      if (t + 16 <= cnt) {
        uint64_t v[2];
        memcpy(v, s + t, 16);
        memcpy(d + t, v, 16);
      } else {
        for (uint32_t i = t; i < cnt; i++) d[i] = s[i]; // a stream's last bytes
      }
    }
    ZW_SYNC();
  }
  ZW_LANES { if (lane < ns && S.hs_pos[lane] != 0) S.fail = 1; }
  ZW_SYNC();
  return !S.fail;
}
// RLE literals need no buffer: the moves below fill
ZFN void zm_rle_literals(ZstdLargeLds&, const ZMemGlobal&, uint32_t) {}

ZFN const uint8_t* zl_literals(const ZstdLargeLds& S, const ZMemGlobal& m) {
  return S.lit_inplace ? m.in + S.lit_off : m.lit;
}

// A placed batch: seq_lp/seq_op hold where each run of literals starts in
// the literals and in the output; every bound has been checked.
template <class M>
ZFN void zm_exec_batch(ZstdLargeLds& S, const M& m, uint32_t cnt, uint32_t zlane) {
  (void)zlane;
  const uint8_t* lit = zl_literals(S, m);
  const uint32_t fill = S.lit_fill, rle = S.lit_rle, lit0 = S.litpos;
  const uint32_t nlit = S.seq_lp[cnt - 1] + S.seq_ll[cnt - 1] - lit0;
  ZW_LANES { // the batch's literals are lit[lit0, +nlit): a byte per lane
    for (uint32_t i = lane; i < nlit; i += 64) {
      const uint32_t lp = lit0 + i;
      uint32_t lo = 0, hi = cnt; // the last run that starts at or below lp
      while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (S.seq_lp[mid] <= lp) lo = mid; else hi = mid;
      }
      m.out[S.seq_op[lo] + (lp - S.seq_lp[lo])] = fill ? (uint8_t)rle : lit[lp];
    }
  }
  ZW_SYNC();
  for (uint32_t k = 0; k < cnt; k++) { // matches in order, the wave on each
    uint32_t ml = S.seq_ml[k];
    const uint32_t off = S.seq_off[k], at = S.seq_op[k] + S.seq_ll[k];
    uint8_t* d = m.out + at;
    const uint32_t pre = zm_dict_part(m, d, at, off, ml, zlane);
    d += pre;
    ml -= pre;
    const uint8_t* s = d - off;
    if (off >= ml && ml >= 128) {
      ZL_COPY(d, s, ml)
    } else {
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
    }
    ZW_SYNC();
  }
}
ZFN void zm_tail_literals(ZstdLargeLds& S, const ZMemGlobal& m, uint32_t rem,
                          uint32_t op, uint32_t zlane) {
  (void)zlane;
  uint8_t* d = m.out + op;
  if (S.lit_fill) {
    const uint32_t v = S.lit_rle;
    ZL_FILL(d, v, rem)
  } else {
    const uint8_t* s = zl_literals(S, m) + S.litpos;
    ZL_COPY(d, s, rem)
  }
  ZW_SYNC();
}
ZFN void zm_plain_block(ZstdLargeLds&, const ZMemGlobal& m, uint32_t type,
                        uint32_t ip, uint32_t op, uint32_t sz, uint32_t zlane) {
  (void)zlane;
  uint8_t* d = m.out + op;
  const uint8_t* s = m.in + ip;
  if (type == 0) {
    ZL_COPY(d, s, sz)
  } else {
    const uint32_t v = s[0];
    ZL_FILL(d, v, sz)
  }
  ZW_SYNC();
}

// The frame m.in[0, n) -> m.out[0, cap); cap <= 0x7fffffff.
ZFN bool zstd_dec_wave_large(ZstdLargeLds& S, const ZMemGlobal& m, uint32_t n,
                             uint32_t cap, uint32_t zlane) {
  return zstd_dec_frame(S, m, n, cap, zlane);
}
#endif // DCW_ZSTD_WAVE

} // namespace dcw
