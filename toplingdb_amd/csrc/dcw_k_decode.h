// dcw_k_decode.h — device error codes and the decode-side kernels.
// A section of the single GPU translation unit: dcw_gpu.hip includes the
// dcw_k_*.h headers in order, inside one unit, so every kernel is defined
// before the host code that launches it.  Not a stand-alone header.
#pragma once
#include "dcw_gpu.h"

#define WAVE 64

namespace dcw {

enum DevErr : uint32_t {
  DE_OK = 0,
  DE_CHECKSUM = 1,
  DE_SNAPPY = 2,
  DE_BLOCK_PARSE = 3,
  DE_UKEY_LEN = 4,     // non-uniform or >16B user keys (round-1 envelope)
  DE_TYPE = 5,         // value type outside {Put, Delete, SingleDelete}
  DE_SD_CONTRACT = 6,  // SingleDelete + Delete mix (Corruption in reference)
  DE_COMPRESS_TYPE = 7,
  DE_PLAN_WIDTH = 8,   // planned block exceeds the emit kernel's entry bound
};

// ------------------------------------------------------------------
// device-side helpers
// ------------------------------------------------------------------
__device__ __forceinline__ bool ent_le(const ulong4& a, const ulong4& b) {
  // (k0,k1,k2) lexicographic; ties -> true (A-side/lower-run wins: stable)
  if (a.x != b.x) return a.x < b.x;
  if (a.y != b.y) return a.y < b.y;
  return a.z <= b.z;
}
__device__ __forceinline__ void set_err(uint32_t* err_flag, uint32_t code) {
  atomicCAS(err_flag, DE_OK, code);
}

// ------------------------------------------------------------------
// decode-side kernels
// ------------------------------------------------------------------
__global__ void k_verify_usize(const uint8_t* __restrict__ blob,
                               const uint64_t* __restrict__ boff,
                               const uint32_t* __restrict__ bsize, uint32_t nblocks,
                               uint32_t checksum_type,
                               const Crc32cTables* __restrict__ crc_tt,
                               uint32_t* __restrict__ usize,
                               uint8_t* __restrict__ btype, uint32_t* err_flag) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nblocks;
       i += gridDim.x * blockDim.x) {
    const uint8_t* p = blob + boff[i];
    uint32_t sz = bsize[i];
    uint8_t type = p[sz];
    uint32_t stored;
    memcpy(&stored, p + sz + 1, 4);
    if (checksum_type != 0) {
      uint32_t actual = block_checksum(checksum_type, crc_tt, p, sz, type);
      if (actual != stored) {
        set_err(err_flag, DE_CHECKSUM);
        return;
      }
    }
    if (type == 0) {
      usize[i] = sz;
    } else if (type == 1) {
      size_t ul = snappy_uncompressed_len(p, sz);
      if (ul == (size_t)-1) {
        set_err(err_flag, DE_SNAPPY);
        return;
      }
      usize[i] = (uint32_t)ul;
    } else {
      set_err(err_flag, DE_COMPRESS_TYPE);
      return;
    }
    btype[i] = type;
  }
}

// one wave per block: raw -> cooperative copy; snappy -> staged through LDS
// (compressed in + decoded out both in LDS, lane 0 runs the serial decoder,
// all lanes copy in/out); oversized blocks fall back to the direct path.
#define DEC_MAX 4992 // 2*(4992+16)*4 waves = 40.1 KB LDS/WG -> 4 WGs (16 decoders)/CU
// (an asymmetric in[3200]+out[4992] layout reaching 20 decoders/CU was
// measured slower end-to-end; LDS staging of BOTH sides is load-bearing)
#define DEC_PAD 16 // slack for the 8/16-byte moves of the fast decoder
struct DecLds {
  uint8_t in[DEC_MAX + DEC_PAD]; // compressed input + decoded output both
  uint8_t out[DEC_MAX + DEC_PAD]; // staged in LDS: the serial byte decoder
                                  // is LDS-latency bound (a global-input
                                  // variant measured ~10% slower)
};

} // namespace dcw
#include "dcw_snap_dec_lds.h"
namespace dcw {

__device__ __forceinline__ void wave_lds_sync2() {
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
}

// Wave-cooperative decoder (DCW_DEC_PIPE=2): all 64 lanes run the tag
// parse in LOCKSTEP (same data, same branches - zero divergence, so the
// serial parse chain is paid once per wave, not once per op), each lane
// keeps every 64th op in registers, and the batch then executes in
// dependency rounds: literals and copies whose source lies wholly below
// the done-prefix frontier run concurrently across lanes; the frontier
// op itself is always executable (pattern doubling reads only its own
// writes and the done region), so progress is guaranteed.  Bounds
// checks are identical to the serial decoder and lane-uniform.
__device__ uint32_t snap_dec_wave(const uint8_t* __restrict__ in, uint32_t n,
                                  uint8_t* __restrict__ out, uint32_t cap,
                                  uint32_t lane) {
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
  uint32_t opos = 0;
  while (ip < n) {
    uint32_t nops = 0;
    uint32_t my_dst = 0, my_src = 0, my_len = 0, my_kind = 0;
    while (ip < n && nops < WAVE) {
      uint64_t h = lds_ld64(in + ip);
      uint8_t tag = (uint8_t)h;
      uint32_t len, srcp, kind;
      if ((tag & 3) == 0) { // literal
        len = (uint32_t)(tag >> 2) + 1;
        uint32_t hb = 1;
        if (len > 60) {
          uint32_t nb = len - 60;
          if (ip + 1 + nb > n) return 0;
          uint32_t lm1 = (uint32_t)((h >> 8) & (0xffffffffull >> (8 * (4 - nb))));
          // a 4-byte length near 2^32 would wrap len / ip + len below
          if (lm1 >= n) return 0;
          len = lm1 + 1;
          hb = 1 + nb;
        }
        ip += hb;
        if (ip + len > n || opos + len > ulen) return 0;
        srcp = ip;
        kind = 1;
        ip += len;
      } else { // copy
        uint32_t offset, hb;
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
        if (offset == 0 || offset > opos || opos + len > ulen) return 0;
        srcp = opos - offset;
        kind = 2;
      }
      if (nops == lane) {
        my_dst = opos;
        my_src = srcp;
        my_len = len;
        my_kind = kind;
      }
      opos += len;
      nops++;
    }
    uint64_t done_mask = 0;
    uint32_t frontier = 0;
    while (frontier < nops) {
      uint32_t fdst = __shfl(my_dst, (int)frontier);
      bool pending = lane < nops && !((done_mask >> lane) & 1);
      bool ready = pending && (my_kind == 1 ||
                               my_src + my_len <= fdst || lane == frontier);
      if (ready) {
        // EXACT-length stores: rounds execute ops out of order, so the
        // serial decoder's 15-byte overshoot would clobber a neighbour
        // op's already-written bytes
        const uint8_t* sbase = my_kind == 1 ? in : out;
        uint32_t offset = my_kind == 1 ? 0xffffffffu : my_dst - my_src;
        uint32_t t = 0;
        if (offset >= 16) {
          for (; t + 16 <= my_len; t += 16) {
            uint64_t a = lds_ld64(sbase + my_src + t);
            uint64_t b = lds_ld64(sbase + my_src + t + 8);
            lds_st64(out + my_dst + t, a);
            lds_st64(out + my_dst + t + 8, b);
          }
          for (; t < my_len; t++) out[my_dst + t] = sbase[my_src + t];
        } else if (offset >= 8) {
          for (; t + 8 <= my_len; t += 8)
            lds_st64(out + my_dst + t, lds_ld64(out + my_src + t));
          for (; t < my_len; t++) out[my_dst + t] = out[my_src + t];
        } else {
          uint32_t o = my_dst, src = my_src, end = my_dst + my_len;
          while (o < end) {
            uint32_t d = o - src;
            if (end - o < 8 || d < 8) {
              if (end - o < 8) { // byte-exact tail
                for (; o < end; o++) out[o] = out[o - offset];
                break;
              }
              lds_st64(out + o, lds_ld64(out + src));
              o += d < end - o ? d : end - o;
            } else {
              // pattern established through o at distance d (a power-of-two
              // multiple of offset): chunk-copy at that distance, byte tail
              uint32_t dist = d;
              for (; o + 8 <= end; o += 8)
                lds_st64(out + o, lds_ld64(out + o - dist));
              for (; o < end; o++) out[o] = out[o - offset];
              break;
            }
          }
        }
      }
      wave_lds_sync2();
      done_mask |= __ballot(ready);
      while (frontier < nops && ((done_mask >> frontier) & 1)) frontier++;
    }
  }
  return opos == ulen ? ulen : 0;
}

__global__ __launch_bounds__(256) void k_decompress(
    const uint8_t* __restrict__ blob, const uint64_t* __restrict__ boff,
    const uint32_t* __restrict__ bsize, const uint8_t* __restrict__ btype,
    const uint64_t* __restrict__ uoff, const uint32_t* __restrict__ usize,
    uint32_t nblocks, uint8_t* __restrict__ ublob, uint32_t* err_flag,
    uint32_t dec_pipe) {
  __shared__ DecLds lds[4];
  uint32_t waves_per_wg = blockDim.x / WAVE;
  uint32_t wid = threadIdx.x / WAVE;
  uint32_t wave = blockIdx.x * waves_per_wg + wid;
  uint32_t lane = threadIdx.x % WAVE;
  uint32_t stride = gridDim.x * waves_per_wg;
  DecLds& L = lds[wid];
  for (uint32_t i = wave; i < nblocks; i += stride) {
    const uint8_t* src = blob + boff[i];
    uint8_t* dst = ublob + uoff[i];
    uint32_t n = bsize[i];
    if (btype[i] == 0) {
      uint32_t pos = lane * 16;
      for (; pos + 16 <= n; pos += WAVE * 16) {
        ulong2 v;
        memcpy(&v, src + pos, 16);
        memcpy(dst + pos, &v, 16);
      }
      if (lane == 0)
        for (uint32_t t = n & ~15u; t < n; t++) dst[t] = src[t];
    } else if (n <= DEC_MAX && usize[i] <= DEC_MAX) {
      // 16-byte staging: byte-granular copies issued ~5000 DS ops per
      // block per wave and saturated the CU's DS issue pipe that the 16
      // resident serial decoders depend on
      for (uint32_t t = lane * 16; t + 16 <= n; t += WAVE * 16) {
        ulong2 v;
        memcpy(&v, src + t, 16);
        memcpy(L.in + t, &v, 16);
      }
      if (lane == 0)
        for (uint32_t t = n & ~15u; t < n; t++) L.in[t] = src[t];
      wave_lds_sync2();
      if (dec_pipe == 2) {
        uint32_t r = snap_dec_wave(L.in, n, L.out, usize[i], lane);
        if (lane == 0 && r != usize[i]) set_err(err_flag, DE_SNAPPY);
      } else if (lane == 0) {
        uint32_t r = dec_pipe ? snap_dec_lds<1>(L.in, n, L.out, usize[i])
                              : snap_dec_lds<0>(L.in, n, L.out, usize[i]);
        if (r != usize[i]) set_err(err_flag, DE_SNAPPY);
      }
      wave_lds_sync2();
      uint32_t un = usize[i];
      for (uint32_t t = lane * 16; t + 16 <= un; t += WAVE * 16) {
        ulong2 v;
        memcpy(&v, L.out + t, 16);
        memcpy(dst + t, &v, 16);
      }
      if (lane == 0)
        for (uint32_t t = un & ~15u; t < un; t++) dst[t] = L.out[t];
      wave_lds_sync2();
    } else {
      if (lane == 0) {
        if (snappy_uncompress(src, n, dst, usize[i]) != usize[i])
          set_err(err_flag, DE_SNAPPY);
      }
    }
  }
}

// Decompress variant 1: LDS stages the DECODED side only; the serial
// decoder reads compressed input straight from global (tag bytes are ~1
// per ~35 output bytes; literal/copy payloads already move as words in
// snappy_uncompress).  Halving the LDS footprint doubles resident
// decoders: 4 waves/WG x 8 WGs/CU = 32 serial decoders per CU.
struct DecLdsOut {
  uint8_t out[DEC_MAX];
};
__global__ __launch_bounds__(256) void k_decompress_v1(
    const uint8_t* __restrict__ blob, const uint64_t* __restrict__ boff,
    const uint32_t* __restrict__ bsize, const uint8_t* __restrict__ btype,
    const uint64_t* __restrict__ uoff, const uint32_t* __restrict__ usize,
    uint32_t nblocks, uint8_t* __restrict__ ublob, uint32_t* err_flag) {
  __shared__ DecLdsOut lds[4];
  uint32_t waves_per_wg = blockDim.x / WAVE;
  uint32_t wid = threadIdx.x / WAVE;
  uint32_t wave = blockIdx.x * waves_per_wg + wid;
  uint32_t lane = threadIdx.x % WAVE;
  uint32_t stride = gridDim.x * waves_per_wg;
  DecLdsOut& L = lds[wid];
  for (uint32_t i = wave; i < nblocks; i += stride) {
    const uint8_t* src = blob + boff[i];
    uint8_t* dst = ublob + uoff[i];
    uint32_t n = bsize[i];
    if (btype[i] == 0) {
      uint32_t pos = lane * 16;
      for (; pos + 16 <= n; pos += WAVE * 16) {
        ulong2 v;
        memcpy(&v, src + pos, 16);
        memcpy(dst + pos, &v, 16);
      }
      if (lane == 0)
        for (uint32_t t = n & ~15u; t < n; t++) dst[t] = src[t];
    } else if (usize[i] <= DEC_MAX) {
      if (lane == 0) {
        if (snappy_uncompress(src, n, L.out, usize[i]) != usize[i])
          set_err(err_flag, DE_SNAPPY);
      }
      wave_lds_sync2();
      uint32_t un = usize[i];
      for (uint32_t t = lane * 4; t < un; t += WAVE * 4) {
        uint32_t chunk = un - t < 4 ? un - t : 4;
        for (uint32_t x = 0; x < chunk; x++) dst[t + x] = L.out[t + x];
      }
      wave_lds_sync2();
    } else {
      if (lane == 0) {
        if (snappy_uncompress(src, n, dst, usize[i]) != usize[i])
          set_err(err_flag, DE_SNAPPY);
      }
    }
  }
}

// Decompress variant 2: no LDS at all — the serial decoder reads global
// and writes global; back-references read recently-written (L1-hot)
// output.  Occupancy is register-bound only.
__global__ __launch_bounds__(256) void k_decompress_v2(
    const uint8_t* __restrict__ blob, const uint64_t* __restrict__ boff,
    const uint32_t* __restrict__ bsize, const uint8_t* __restrict__ btype,
    const uint64_t* __restrict__ uoff, const uint32_t* __restrict__ usize,
    uint32_t nblocks, uint8_t* __restrict__ ublob, uint32_t* err_flag) {
  uint32_t waves_per_wg = blockDim.x / WAVE;
  uint32_t wave = blockIdx.x * waves_per_wg + threadIdx.x / WAVE;
  uint32_t lane = threadIdx.x % WAVE;
  uint32_t stride = gridDim.x * waves_per_wg;
  for (uint32_t i = wave; i < nblocks; i += stride) {
    const uint8_t* src = blob + boff[i];
    uint8_t* dst = ublob + uoff[i];
    uint32_t n = bsize[i];
    if (btype[i] == 0) {
      uint32_t pos = lane * 16;
      for (; pos + 16 <= n; pos += WAVE * 16) {
        ulong2 v;
        memcpy(&v, src + pos, 16);
        memcpy(dst + pos, &v, 16);
      }
      if (lane == 0)
        for (uint32_t t = n & ~15u; t < n; t++) dst[t] = src[t];
    } else if (lane == 0) {
      if (snappy_uncompress(src, n, dst, usize[i]) != usize[i])
        set_err(err_flag, DE_SNAPPY);
    }
  }
}

__global__ void k_num_restarts(const uint8_t* __restrict__ ublob,
                               const uint64_t* __restrict__ uoff,
                               const uint32_t* __restrict__ usize, uint32_t nblocks,
                               uint32_t* __restrict__ nrestarts, uint32_t* err_flag) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nblocks;
       i += gridDim.x * blockDim.x) {
    uint32_t us = usize[i];
    if (us < 8) {
      set_err(err_flag, DE_BLOCK_PARSE);
      return;
    }
    uint32_t footer;
    memcpy(&footer, ublob + uoff[i] + us - 4, 4);
    uint32_t nr = footer & 0x7fffffffu;
    if (4ull + 4ull * nr + 4ull > us) {
      set_err(err_flag, DE_BLOCK_PARSE);
      return;
    }
    nrestarts[i] = nr;
  }
}

// walk one restart interval: count entries (pass 1) or decode them (pass 2)
__device__ __forceinline__ int interval_bounds(
    const uint8_t* ublk, uint32_t usize, uint32_t nr, uint32_t j, uint32_t* beg,
    uint32_t* end) {
  const uint8_t* rst = ublk + usize - 4 - 4 * nr;
  uint32_t b, e;
  memcpy(&b, rst + 4 * j, 4);
  if (j + 1 < nr)
    memcpy(&e, rst + 4 * (j + 1), 4);
  else
    e = (uint32_t)(usize - 4 - 4 * nr);
  if (b > e || e > usize) return -1;
  *beg = b;
  *end = e;
  return 0;
}

// 16-byte register window over a sequential in-block scan.  The interval
// walkers consume ~4 header bytes then skip ~100 value bytes; byte-granular
// loads at that stride re-fetched each cache line ~2.6-5.5x (round-1 PMC,
// profiles/pmc_hbm_traffic_r01_v4.txt).  Two u64 loads per 16 consumed
// bytes at UNCHANGED thread parallelism cut the per-line touch count ~8x.
// fill() may read up to 15 B past an interval/block end: d_ublob is
// allocated with >=64 B of slack (DevBuf::reserve), so the loads stay in bounds.
struct ByteWin {
  const uint8_t* base;
  uint64_t w0, w1;
  uint32_t off;
  __device__ __forceinline__ void fill(uint32_t o) {
    off = o;
    memcpy(&w0, base + o, 8);
    memcpy(&w1, base + o + 8, 8);
  }
  __device__ __forceinline__ uint8_t at(uint32_t pos) {
    uint32_t d = pos - off;
    if (d >= 16) {
      fill(pos);
      d = 0;
    }
    return d < 8 ? (uint8_t)(w0 >> (8 * d)) : (uint8_t)(w1 >> (8 * (d - 8)));
  }
};

// varint32_get over the window; advances pos.  Same accept/reject set as
// the pointer variant (dcw_common.h varint32_get).
__device__ __forceinline__ bool win_varint32(ByteWin& W, uint32_t& pos,
                                             uint32_t lim, uint32_t* v) {
  uint32_t r = 0, sh = 0;
  while (pos < lim && sh <= 28) {
    uint8_t b = W.at(pos);
    pos++;
    r |= (uint32_t)(b & 0x7f) << sh;
    if (!(b & 0x80)) {
      *v = r;
      return true;
    }
    sh += 7;
  }
  return false;
}

__global__ void k_count_entries(const uint8_t* __restrict__ ublob,
                                const uint64_t* __restrict__ uoff,
                                const uint32_t* __restrict__ usize,
                                const uint32_t* __restrict__ nrestarts,
                                const uint32_t* __restrict__ iv_block,
                                const uint32_t* __restrict__ iv_local,
                                uint32_t nintervals, uint32_t* __restrict__ iv_cnt,
                                uint32_t* err_flag) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nintervals;
       i += gridDim.x * blockDim.x) {
    uint32_t b = iv_block[i];
    const uint8_t* ublk = ublob + uoff[b];
    uint32_t beg, end;
    if (interval_bounds(ublk, usize[b], nrestarts[b], iv_local[i], &beg, &end) != 0) {
      set_err(err_flag, DE_BLOCK_PARSE);
      return;
    }
    ByteWin W;
    W.base = ublk;
    if (beg < end) W.fill(beg);
    uint32_t pos = beg;
    uint32_t n = 0;
    while (pos < end) {
      uint32_t shared, non_shared, vlen;
      if (!win_varint32(W, pos, end, &shared)) break;
      if (!win_varint32(W, pos, end, &non_shared)) break;
      if (!win_varint32(W, pos, end, &vlen)) break;
      // 64-bit: a corrupt length must not wrap pos back below end (the walk
      // would never terminate); same check as k_decode_entries
      uint64_t nxt = (uint64_t)pos + non_shared + vlen;
      if (nxt > end) {
        set_err(err_flag, DE_BLOCK_PARSE);
        return;
      }
      pos = (uint32_t)nxt;
      n++;
    }
    iv_cnt[i] = n;
  }
}

// Register-resident key state: the internal key (user key <= 16 B + 8 B tag)
// lives in three u64s — kb0/kb1 = key bytes 0..7 / 8..15 in MEMORY order
// (little-endian u64 of the byte string), tail = bytes 16..klen.  Dynamic
// byte indexing through shifts only: no per-thread scratch array.
__device__ __forceinline__ void key_set_byte(uint64_t& kb0, uint64_t& kb1,
                                             uint64_t& tail, uint32_t j,
                                             uint8_t v) {
  uint64_t m = 0xffull;
  uint64_t x = (uint64_t)v;
  if (j < 8) {
    kb0 = (kb0 & ~(m << (8 * j))) | (x << (8 * j));
  } else if (j < 16) {
    kb1 = (kb1 & ~(m << (8 * (j - 8)))) | (x << (8 * (j - 8)));
  } else {
    tail = (tail & ~(m << (8 * (j - 16)))) | (x << (8 * (j - 16)));
  }
}

__global__ void k_decode_entries(
    const uint8_t* __restrict__ ublob, const uint64_t* __restrict__ uoff,
    const uint32_t* __restrict__ usize, const uint32_t* __restrict__ nrestarts,
    const uint32_t* __restrict__ iv_block, const uint32_t* __restrict__ iv_local,
    const uint32_t* __restrict__ iv_base, uint32_t nintervals,
    ulong4* __restrict__ ents, uint64_t* __restrict__ voff,
    uint32_t* __restrict__ vlen_out, uint8_t* __restrict__ klen_out,
    uint32_t* __restrict__ ukey_len_probe, uint32_t* err_flag) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nintervals;
       i += gridDim.x * blockDim.x) {
    uint32_t b = iv_block[i];
    const uint8_t* ublk = ublob + uoff[b];
    uint32_t beg, end;
    if (interval_bounds(ublk, usize[b], nrestarts[b], iv_local[i], &beg, &end) != 0)
      return;
    ByteWin W;
    W.base = ublk;
    if (beg < end) W.fill(beg);
    uint32_t pos = beg;
    uint64_t kb0 = 0, kb1 = 0, ktail = 0; // key bytes in registers
    uint32_t klen = 0;
    uint32_t out = iv_base[i];
    uint32_t probed_ulen = 0xffffffffu;
    while (pos < end) {
      uint32_t shared, non_shared, vl;
      if (!win_varint32(W, pos, end, &shared)) break;
      if (!win_varint32(W, pos, end, &non_shared)) break;
      if (!win_varint32(W, pos, end, &vl)) break;
      if (shared + non_shared > 24) {
        // beyond the fast path's 24-byte ikey registers: the host retries
        // in general-key mode (could still be corruption — the general
        // decode re-validates against DCW_GKEY_MAX)
        set_err(err_flag, DE_UKEY_LEN);
        return;
      }
      if (shared > klen || (uint64_t)pos + non_shared + vl > end) {
        set_err(err_flag, DE_BLOCK_PARSE);
        return;
      }
      for (uint32_t t = 0; t < non_shared; t++)
        key_set_byte(kb0, kb1, ktail, shared + t, W.at(pos + t));
      klen = shared + non_shared;
      pos += non_shared;
      if (klen < 9) {
        set_err(err_flag, DE_BLOCK_PARSE);
        return;
      }
      uint32_t ulen = klen - 8;
      if (ulen > 16) {
        set_err(err_flag, DE_UKEY_LEN);
        return;
      }
      if (probed_ulen != ulen) {
        uint32_t expect = atomicCAS(ukey_len_probe, 0xffffffffu, ulen);
        if (expect != 0xffffffffu && expect != ulen) {
          set_err(err_flag, DE_UKEY_LEN);
          return;
        }
        probed_ulen = ulen;
      }
      // tag = 8 LE bytes starting at byte ulen of the key
      uint64_t tag;
      if (ulen == 16) {
        tag = ktail;
      } else if (ulen >= 8) {
        uint32_t sh = 8 * (ulen - 8);
        tag = sh ? ((kb1 >> sh) | (ktail << (64 - sh))) : kb1;
      } else {
        uint32_t sh = 8 * ulen;
        tag = sh ? ((kb0 >> sh) | (kb1 << (64 - sh))) : kb0;
      }
      uint8_t vt = (uint8_t)tag;
      if (!(vt == kTypeValue || vt == kTypeDeletion || vt == kTypeSingleDeletion)) {
        set_err(err_flag, DE_TYPE);
        return;
      }
      // normkey: big-endian words of the zero-padded user key
      uint64_t u0, u1;
      if (ulen >= 8) {
        u0 = kb0;
        uint32_t rem = ulen - 8; // bytes of user key in kb1
        u1 = rem ? (kb1 & ((rem == 8) ? ~0ull : ((1ull << (8 * rem)) - 1))) : 0;
      } else {
        u0 = ulen ? (kb0 & ((1ull << (8 * ulen)) - 1)) : 0;
        u1 = 0;
      }
      ents[out] = make_ulong4(__builtin_bswap64(u0), __builtin_bswap64(u1),
                              ~tag, out);
      voff[out] = uoff[b] + pos;
      vlen_out[out] = vl;
      klen_out[out] = (uint8_t)klen;
      pos += vl;
      out++;
    }
  }
}

// ---------------- general key shapes (mixed/long user keys) ----------------
// The fast path packs the whole <=16 B uniform user key into the normkey
// (k0,k1).  GENERAL mode (mixed lengths or 16 < ukey <= DCW_GKEY_MAX)
// keeps (k0,k1) as the zero-padded 16-byte PREFIX and stores the FULL
// user key in a fixed-stride side table `kext` indexed by the entry's
// payload index w; comparisons gather the tail only on prefix ties
// (db/dbformat.h:1057-1096 arbitrary-length bytewise contract).
// DCW_GKEY_MAX / DCW_GKEY_STRIDE: dcw_common.h.

// full user-key bytewise compare from the side table (klen = ikey length)
__device__ __forceinline__ int gkey_cmp(const uint8_t* __restrict__ kext,
                                        const uint8_t* __restrict__ klen,
                                        uint64_t wa, uint64_t wb) {
  const uint8_t* A = kext + wa * DCW_GKEY_STRIDE;
  const uint8_t* B = kext + wb * DCW_GKEY_STRIDE;
  uint32_t la = klen[wa] - 8, lb = klen[wb] - 8;
  uint32_t m = la < lb ? la : lb;
  uint32_t t = 0;
  for (; t + 8 <= m; t += 8) {
    uint64_t x, y;
    memcpy(&x, A + t, 8);
    memcpy(&y, B + t, 8);
    if (x != y) {
      x = __builtin_bswap64(x);
      y = __builtin_bswap64(y);
      return x < y ? -1 : 1;
    }
  }
  for (; t < m; t++)
    if (A[t] != B[t]) return A[t] < B[t] ? -1 : 1;
  if (la != lb) return la < lb ? -1 : 1;
  return 0;
}

// general entry order: prefix words, then full-key gather, then ~tag
__device__ __forceinline__ bool ent_le_g(const ulong4& a, const ulong4& b,
                                         const uint8_t* __restrict__ kext,
                                         const uint8_t* __restrict__ klen) {
  if (a.x != b.x) return a.x < b.x;
  if (a.y != b.y) return a.y < b.y;
  if (kext) {
    int c = gkey_cmp(kext, klen, a.w, b.w);
    if (c) return c < 0;
  }
  return a.z <= b.z;
}

// general decode: running key kept in a local buffer; full ukey bytes go
// to the side table, prefix normkey to the entry array
__global__ void k_decode_entries_g(
    const uint8_t* __restrict__ ublob, const uint64_t* __restrict__ uoff,
    const uint32_t* __restrict__ usize, const uint32_t* __restrict__ nrestarts,
    const uint32_t* __restrict__ iv_block, const uint32_t* __restrict__ iv_local,
    const uint32_t* __restrict__ iv_base, uint32_t nintervals,
    ulong4* __restrict__ ents, uint64_t* __restrict__ voff,
    uint32_t* __restrict__ vlen_out, uint8_t* __restrict__ klen_out,
    uint8_t* __restrict__ kext, uint32_t* err_flag) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nintervals;
       i += gridDim.x * blockDim.x) {
    uint32_t b = iv_block[i];
    const uint8_t* ublk = ublob + uoff[b];
    uint32_t beg, end;
    if (interval_bounds(ublk, usize[b], nrestarts[b], iv_local[i], &beg, &end) != 0)
      return;
    ByteWin W;
    W.base = ublk;
    if (beg < end) W.fill(beg);
    uint32_t pos = beg;
    uint8_t cur[DCW_GKEY_MAX + 8];
    uint32_t klen = 0;
    uint32_t out = iv_base[i];
    while (pos < end) {
      uint32_t shared, non_shared, vl;
      if (!win_varint32(W, pos, end, &shared)) break;
      if (!win_varint32(W, pos, end, &non_shared)) break;
      if (!win_varint32(W, pos, end, &vl)) break;
      if (shared > klen || shared + non_shared > DCW_GKEY_MAX + 8 ||
          (uint64_t)pos + non_shared + vl > end) {
        set_err(err_flag,
                shared + non_shared > DCW_GKEY_MAX + 8 ? DE_UKEY_LEN
                                                       : DE_BLOCK_PARSE);
        return;
      }
      for (uint32_t t = 0; t < non_shared; t++) cur[shared + t] = W.at(pos + t);
      klen = shared + non_shared;
      pos += non_shared;
      if (klen < 9) {
        set_err(err_flag, DE_BLOCK_PARSE);
        return;
      }
      uint32_t ulen = klen - 8;
      uint64_t tag;
      memcpy(&tag, cur + ulen, 8);
      uint8_t vt = (uint8_t)tag;
      if (!(vt == kTypeValue || vt == kTypeDeletion || vt == kTypeSingleDeletion)) {
        set_err(err_flag, DE_TYPE);
        return;
      }
      // prefix normkey: first 16 bytes zero-padded, big-endian words
      uint64_t u0 = 0, u1 = 0;
      uint32_t p0 = ulen < 8 ? ulen : 8;
      memcpy(&u0, cur, 8);
      if (ulen < 8) u0 &= p0 ? ((p0 == 8) ? ~0ull : ((1ull << (8 * p0)) - 1)) : 0;
      if (ulen > 8) {
        uint32_t p1 = ulen - 8 < 8 ? ulen - 8 : 8;
        memcpy(&u1, cur + 8, 8);
        u1 &= (p1 == 8) ? ~0ull : ((1ull << (8 * p1)) - 1);
      }
      ents[out] = make_ulong4(__builtin_bswap64(u0), __builtin_bswap64(u1),
                              ~tag, out);
      // full ukey into the side table (zero-pad the slot tail)
      uint8_t* slot = kext + (uint64_t)out * DCW_GKEY_STRIDE;
      for (uint32_t t = 0; t < ulen; t++) slot[t] = cur[t];
      for (uint32_t t = ulen; t < DCW_GKEY_STRIDE; t++) slot[t] = 0;
      voff[out] = uoff[b] + pos;
      vlen_out[out] = vl;
      klen_out[out] = (uint8_t)klen;
      pos += vl;
      out++;
    }
  }
}

// flush offload input: one thread per raw KV record.
// Record: [klen u32][ikey][vlen u32][value]; offs[i] = record offset,
// offs[n] = blob size.  general: keys > 16 B / mixed via the side table.
__global__ void k_decode_flush(const uint8_t* __restrict__ blob,
                               const uint64_t* __restrict__ offs, uint64_t n,
                               int general, uint32_t uniform_ulen,
                               ulong4* __restrict__ ents,
                               uint64_t* __restrict__ voff,
                               uint32_t* __restrict__ vlen_out,
                               uint8_t* __restrict__ klen_out,
                               uint8_t* __restrict__ kext, uint32_t* err_flag) {
  for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint8_t* p = blob + offs[i];
    const uint8_t* lim = blob + offs[i + 1];
    uint32_t klen, vl;
    memcpy(&klen, p, 4);
    const uint8_t* key = p + 4;
    memcpy(&vl, key + klen, 4);
    if (p + 8 + klen + vl > lim || klen < 9 ||
        klen > (general ? DCW_GKEY_MAX + 8u : 24u)) {
      set_err(err_flag, DE_BLOCK_PARSE);
      return;
    }
    uint32_t ulen = klen - 8;
    if (!general && ulen != uniform_ulen) {
      set_err(err_flag, DE_UKEY_LEN);
      return;
    }
    uint64_t tag;
    memcpy(&tag, key + ulen, 8);
    uint8_t vt = (uint8_t)tag;
    if (!(vt == kTypeValue || vt == kTypeDeletion || vt == kTypeSingleDeletion)) {
      set_err(err_flag, DE_TYPE);
      return;
    }
    uint64_t u0 = 0, u1 = 0;
    for (uint32_t t = 0; t < ulen && t < 8; t++)
      u0 |= (uint64_t)key[t] << (8 * t);
    for (uint32_t t = 8; t < ulen && t < 16; t++)
      u1 |= (uint64_t)key[t] << (8 * (t - 8));
    ents[i] = make_ulong4(__builtin_bswap64(u0), __builtin_bswap64(u1), ~tag,
                          i);
    if (general) {
      uint8_t* slot = kext + i * (uint64_t)DCW_GKEY_STRIDE;
      for (uint32_t t = 0; t < ulen; t++) slot[t] = key[t];
      for (uint32_t t = ulen; t < DCW_GKEY_STRIDE; t++) slot[t] = 0;
    }
    voff[i] = (uint64_t)(key + klen + 4 - blob);
    vlen_out[i] = vl;
    klen_out[i] = (uint8_t)klen;
  }
}

} // namespace dcw
