// dcw_k_emit.h — block emit, snappy encode, checksum, pack, plan and stats kernels.
// A section of the single GPU translation unit: dcw_gpu.hip includes the
// dcw_k_*.h headers in order, inside one unit, so every kernel is defined
// before the host code that launches it.  Not a stand-alone header.
#pragma once
#include "dcw_snap_enc_big.h"

namespace dcw {

__device__ __forceinline__ void build_ikey(uint64_t k0, uint64_t k1, uint64_t tag,
                                           uint32_t klen, uint8_t* out) {
  uint64_t b0 = __builtin_bswap64(k0), b1 = __builtin_bswap64(k1);
  memcpy(out, &b0, 8);
  memcpy(out + 8, &b1, 8);
  memcpy(out + (klen - 8), &tag, 8);
}
// internal key of survivor i: fast path from the normkey, general path
// from the full-key side table (out must hold DCW_GKEY_MAX+8)
__device__ __forceinline__ void load_ikey(
    uint64_t k0, uint64_t k1, uint64_t tag, uint32_t klen,
    const uint8_t* __restrict__ kext, const uint32_t* __restrict__ s_w,
    uint64_t i, uint8_t* out) {
  if (!kext) {
    build_ikey(k0, k1, tag, klen, out);
    return;
  }
  const uint8_t* slot = kext + (uint64_t)s_w[i] * 48u;
  uint32_t ulen = klen - 8;
  for (uint32_t t = 0; t < ulen; t++) out[t] = slot[t];
  memcpy(out + ulen, &tag, 8);
}

__global__ void k_shared_prefix(const uint64_t* __restrict__ s_k0,
                                const uint64_t* __restrict__ s_k1,
                                const uint64_t* __restrict__ s_tag,
                                const uint8_t* __restrict__ s_klen, uint64_t n,
                                const uint8_t* __restrict__ kext,
                                const uint32_t* __restrict__ s_w,
                                uint8_t* __restrict__ s_shared) {
  for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    if (i == 0) {
      s_shared[0] = 0;
      continue;
    }
    uint8_t a[DCW_GKEY_MAX + 8], b[DCW_GKEY_MAX + 8];
    uint32_t ka = s_klen[i - 1], kb = s_klen[i];
    load_ikey(s_k0[i - 1], s_k1[i - 1], s_tag[i - 1], ka, kext, s_w, i - 1, a);
    load_ikey(s_k0[i], s_k1[i], s_tag[i], kb, kext, s_w, i, b);
    uint32_t m = ka < kb ? ka : kb;
    uint32_t s = 0;
    while (s < m && a[s] == b[s]) s++;
    s_shared[i] = (uint8_t)s;
  }
}

// ------------------------------------------------------------------
// emit / compress / checksum / pack
// ------------------------------------------------------------------
struct EmitBlockDesc {
  uint32_t first;     // survivor index of first entry (relative to chunk base added on host)
  uint32_t count;
  uint32_t unc_size;  // total uncompressed block size (with restarts+footer)
  uint32_t num_restarts;
  uint64_t uout;      // offset into ucblob
  uint64_t cout;      // offset of the block's compressed-output slot in cblob
};

// one workgroup per block; thread 0 walks the block's entry sizes into an
// LDS offset table (<=512 entries per 4 KiB-class block), then all threads
// encode their entries.  s_shared is the adjacent-survivor prefix from
// k_shared_prefix (shared forced 0 at restart points).
#define EMIT_MAX_ENTRIES 2048
__global__ void k_emit(const EmitBlockDesc* __restrict__ bds, uint32_t nblocks,
                       const uint64_t* __restrict__ s_k0,
                       const uint64_t* __restrict__ s_k1,
                       const uint64_t* __restrict__ s_tag,
                       const uint64_t* __restrict__ s_voff,
                       const uint32_t* __restrict__ s_vlen,
                       const uint8_t* __restrict__ s_klen,
                       const uint8_t* __restrict__ s_shared,
                       const uint8_t* __restrict__ ublob,
                       uint8_t* __restrict__ ucblob, uint32_t restart_interval,
                       const uint8_t* __restrict__ kext,
                       const uint32_t* __restrict__ s_w, uint32_t* err_flag) {
  __shared__ uint32_t offs[EMIT_MAX_ENTRIES];
  __shared__ uint32_t esz[EMIT_MAX_ENTRIES];
  for (uint32_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
    EmitBlockDesc d = bds[b];
    uint8_t* out = ucblob + d.uout;
    if (d.count > EMIT_MAX_ENTRIES) {
      if (threadIdx.x == 0) set_err(err_flag, DE_BLOCK_PARSE);
      __syncthreads();
      continue;
    }
    // per-entry encoded sizes in parallel (the only cross-entry state,
    // the shared prefix, is already in s_shared); thread 0 then runs the
    // short LDS-only prefix walk
    for (uint32_t li = threadIdx.x; li < d.count; li += blockDim.x) {
      uint32_t i = d.first + li;
      uint32_t shared = (li % restart_interval == 0) ? 0 : s_shared[i];
      uint32_t klen = s_klen[i];
      uint32_t vl = s_vlen[i];
      esz[li] = varint_len(shared) + varint_len(klen - shared) +
                varint_len(vl) + (klen - shared) + vl;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t off = 0;
      for (uint32_t li = 0; li < d.count; li++) {
        offs[li] = off;
        off += esz[li];
      }
    }
    __syncthreads();
    for (uint32_t li = threadIdx.x; li < d.count; li += blockDim.x) {
      uint32_t i = d.first + li;
      uint32_t klen = s_klen[i];
      uint8_t key[DCW_GKEY_MAX + 8];
      load_ikey(s_k0[i], s_k1[i], s_tag[i], klen, kext, s_w, i, key);
      uint32_t shared = (li % restart_interval == 0) ? 0 : s_shared[i];
      uint32_t non_shared = klen - shared;
      uint32_t vl = s_vlen[i];
      uint8_t* p = out + offs[li];
      p += varint32_put(p, shared);
      p += varint32_put(p, non_shared);
      p += varint32_put(p, vl);
      for (uint32_t t = 0; t < non_shared; t++) p[t] = key[shared + t];
      p += non_shared;
      const uint8_t* src = ublob + s_voff[i];
      for (uint32_t t = 0; t < vl; t++) p[t] = src[t];
    }
    if (threadIdx.x == 0) {
      // restart array + packed footer (data_block_footer.cc:24-39)
      uint32_t body = d.unc_size - 4 - 4 * d.num_restarts;
      uint8_t* tail = out + body;
      uint32_t r0 = 0;
      memcpy(tail, &r0, 4);
      for (uint32_t j = 1; j < d.num_restarts; j++) {
        uint32_t off = offs[j * restart_interval];
        memcpy(tail + 4 * j, &off, 4);
      }
      uint32_t footer = d.num_restarts; // kDataBlockBinarySearch
      memcpy(tail + 4 * d.num_restarts, &footer, 4);
    }
    __syncthreads();
  }
}

// snappy encode, spec v4: one wave per 4 KiB-class block, WAVE-PARALLEL —
// the spec's first-occurrence hash table is order-independent (min position
// per slot), so all 64 lanes build it together with LDS atomicMin, and the
// spec's fixed segmentation (max(16, ceil(n/64)) bytes) gives every lane an
// independent greedy segment to encode.  Fragments are staged in per-lane
// private buffers, laid out with a wave prefix sum (shfl), and copied to
// the block's output slot.  The segment encoder itself is
// dcw::snap_encode_segment — the SAME function the host C++ restatement
// runs, so device/host byte-parity holds by construction.
#define SNAP_MAX_UNC 16384 // larger blocks go to k_compress_large (below)
#define SNAP_MAX_OUT (32 + SNAP_MAX_UNC + SNAP_MAX_UNC / 6)
#define SNAP_FRAG_MAX 304 // worst-case encode of one <=256 B segment

// wave-internal LDS ordering: drain DS ops + stop compiler reordering
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_s_waitcnt(0); // lgkmcnt(0) & vmcnt(0)
  __builtin_amdgcn_wave_barrier();
}

// Device specialization of dcw::snap_encode_segment with identical output
// bytes: literal copies run 4 bytes at a time and match extension compares
// 4-byte words with ctz — only the data movement differs from the shared
// host restatement, never the emitted stream.
__device__ __forceinline__ uint8_t* snap_emit_literal4v(uint8_t* op,
                                                        const uint8_t* lit,
                                                        uint32_t len) {
  if (len == 0) return op;
  uint32_t n = len - 1;
  if (n < 60) {
    *op++ = (uint8_t)(n << 2);
  } else { // len <= SNAP_FRAG_MAX < 256+1 -> single extra byte
    *op++ = (uint8_t)(60 << 2);
    *op++ = (uint8_t)n;
  }
  uint32_t t = 0;
  for (; t + 4 <= len; t += 4) {
    uint32_t v = load32(lit + t);
    memcpy(op + t, &v, 4);
  }
  for (; t < len; t++) op[t] = lit[t];
  return op + len;
}
template <typename TAB>
__device__ __forceinline__ uint8_t* snap_encode_segment_dev(
    const uint8_t* __restrict__ in, uint32_t s0, uint32_t s1,
    const TAB* __restrict__ tab, uint8_t* op) {
  // TAB = uint32_t or uint16_t: the table stores the same first-occurrence
  // (minimum) positions either way, so the emitted stream is identical
  const uint32_t kNone = (uint32_t)(TAB)~(TAB)0;
  uint32_t lit = s0, p = s0;
  while (p + 4 <= s1) {
    uint32_t w = load32(in + p);
    uint32_t h = (w * kSnapHashMul) >> (32 - kSnapHashBits);
    uint32_t c = tab[h];
    if (c != kNone && c < p && load32(in + c) == w) {
      uint32_t l = 4;
      while (p + l + 4 <= s1) {
        uint32_t a = load32(in + c + l);
        uint32_t bz = load32(in + p + l);
        uint32_t x = a ^ bz;
        if (x) {
          l += __builtin_ctz(x) >> 3;
          goto ext_done;
        }
        l += 4;
      }
      while (p + l < s1 && in[c + l] == in[p + l]) l++;
    ext_done:
      op = snap_emit_literal4v(op, in + lit, p - lit);
      op = snap_emit_copy(op, p - c, l);
      p += l;
      lit = p;
    } else {
      p++;
    }
  }
  return snap_emit_literal4v(op, in + lit, s1 - lit);
}

// min-position insert into a u16 table half-word: CAS on the containing
// aligned u32 keeps atomicMin's exact semantics (valid positions are
// <= SNAP_MAX_UNC-4 < 0xffff, so the sentinel never collides)
__device__ __forceinline__ void lds_min_u16(uint16_t* tab, uint32_t h,
                                            uint32_t p) {
  uint32_t* w = (uint32_t*)tab + (h >> 1);
  uint32_t sh = (h & 1u) * 16;
  uint32_t old = *(volatile uint32_t*)w;
  for (;;) {
    if (p >= ((old >> sh) & 0xffffu)) return;
    uint32_t neu = (old & ~(0xffffu << sh)) | (p << sh);
    uint32_t got = atomicCAS(w, old, neu);
    if (got == old) return;
    old = got;
  }
}

__global__ __launch_bounds__(256, 8) void k_compress(
    const EmitBlockDesc* __restrict__ bds, uint32_t nblocks,
    const uint8_t* __restrict__ ucblob, uint8_t* __restrict__ cblob,
    uint32_t* __restrict__ bsize, uint8_t* __restrict__ btype) {
  // u16 positions halve the table to 4 KiB per wave: 16 KiB per
  // workgroup lifts LDS-limited occupancy 20 -> 28 waves/CU (SGPR-bound),
  // which is what a latency-chain-bound kernel wants; emitted bytes are
  // unchanged (same min-position table content)
  __shared__ uint16_t tabs[4][1u << kSnapHashBits]; // 4 KiB per wave
  uint32_t wid = threadIdx.x / WAVE;  // wave within workgroup
  uint32_t lane = threadIdx.x % WAVE;
  uint32_t waves = blockDim.x / WAVE;
  uint16_t* tab = tabs[wid];
  for (uint32_t b = blockIdx.x * waves + wid; b < nblocks;
       b += gridDim.x * waves) {
    EmitBlockDesc d = bds[b];
    if (d.unc_size > SNAP_MAX_UNC) continue; // k_compress_large's block
    const uint8_t* gin = ucblob + d.uout;
    uint32_t n = d.unc_size;
    {
      uint32_t* tw = (uint32_t*)tab;
      for (uint32_t t = lane; t < (1u << kSnapHashBits) / 2; t += WAVE)
        tw[t] = 0xffffffffu;
    }
    wave_lds_sync();
    for (uint32_t p = lane; p + 4 <= n; p += WAVE) {
      uint32_t h = (load32(gin + p) * kSnapHashMul) >> (32 - kSnapHashBits);
      lds_min_u16(tab, h, p);
    }
    wave_lds_sync();
    uint32_t seg = (uint32_t)snap_segment_size(n);
    uint32_t s0 = lane * seg;
    uint8_t frag[SNAP_FRAG_MAX];
    uint32_t fl = 0;
    if (s0 < n) {
      uint32_t s1 = s0 + seg < n ? s0 + seg : n;
      uint8_t* e = snap_encode_segment_dev(gin, s0, s1, tab, frag);
      fl = (uint32_t)(e - frag);
    }
    // exclusive prefix of fragment sizes across the wave
    uint32_t inc = fl;
    for (int sh = 1; sh < WAVE; sh <<= 1) {
      uint32_t v = __shfl_up(inc, sh);
      if ((int)lane >= sh) inc += v;
    }
    uint32_t total = __shfl(inc, WAVE - 1);
    uint32_t excl = inc - fl;
    uint8_t* gout = cblob + d.cout;
    uint8_t hdr[5];
    uint32_t hl = varint32_put(hdr, n); // lane-uniform
    if (lane == 0)
      for (uint32_t t = 0; t < hl; t++) gout[t] = hdr[t];
    {
      uint8_t* o2 = gout + hl + excl;
      uint32_t t = 0;
      for (; t + 4 <= fl; t += 4) { // misaligned dword stores are fine on gfx950
        uint32_t v;
        memcpy(&v, frag + t, 4);
        memcpy(o2 + t, &v, 4);
      }
      for (; t < fl; t++) o2[t] = frag[t];
    }
    if (lane == 0) {
      uint32_t cn = hl + total;
      // GoodCompressionRatio, default max_compressed_bytes_per_kb=896
      if (cn <= (((uint64_t)896 * n) >> 10)) {
        bsize[b] = cn;
        btype[b] = 1;
      } else {
        bsize[b] = n;
        btype[b] = 0;
      }
    }
    wave_lds_sync();
  }
}

// ---- two-pass compress variants ----
// Pass 1 measures each lane's fragment length (no stores), a shfl prefix
// sum places the fragments, pass 2 re-runs the SAME segment encoder
// writing directly to the block's output slot.  Removes the per-lane
// private fragment buffer entirely: no scratch write+read traffic, no
// 304 B/lane register/scratch footprint, and incompressible blocks skip
// the output writes (the ratio check runs before pass 2).
__device__ __forceinline__ uint32_t snap_lit_len(uint32_t n) {
  // mirrors snap_emit_literal4v: 1-byte header below 60, else 2 (len<=256)
  return n == 0 ? 0 : (n <= 60 ? 1 + n : 2 + n);
}
__device__ __forceinline__ uint32_t snap_copy_len(uint32_t offset, uint32_t len) {
  // mirrors snap_emit_copy's chunking exactly
  uint32_t c = 0;
  while (len > 0) {
    if (len >= 4 && len <= 11 && offset < 2048) return c + 2;
    uint32_t chunk = len > 64 ? 64 : len;
    if (len - chunk > 0 && len - chunk < 4) chunk = len - 4;
    c += 3;
    len -= chunk;
  }
  return c;
}
template <typename TAB>
__device__ __forceinline__ uint32_t snap_measure_segment_dev(
    const uint8_t* __restrict__ in, uint32_t s0, uint32_t s1,
    const TAB* __restrict__ tab) {
  const uint32_t kNone = (uint32_t)(TAB)~(TAB)0;
  uint32_t lit = s0, p = s0, out = 0;
  while (p + 4 <= s1) {
    uint32_t w = load32(in + p);
    uint32_t h = (w * kSnapHashMul) >> (32 - kSnapHashBits);
    uint32_t c = tab[h];
    if (c != kNone && c < p && load32(in + c) == w) {
      uint32_t l = 4;
      while (p + l + 4 <= s1) {
        uint32_t a = load32(in + c + l);
        uint32_t bz = load32(in + p + l);
        uint32_t x = a ^ bz;
        if (x) {
          l += __builtin_ctz(x) >> 3;
          goto mext_done;
        }
        l += 4;
      }
      while (p + l < s1 && in[c + l] == in[p + l]) l++;
    mext_done:
      out += snap_lit_len(p - lit) + snap_copy_len(p - c, l);
      p += l;
      lit = p;
    } else {
      p++;
    }
  }
  return out + snap_lit_len(s1 - lit);
}

// Single-pass wave-parallel compress with the block staged in LDS: the
// encoder's per-iteration dependent chain (load -> hash -> table probe ->
// candidate compare) runs at LDS latency instead of vmem latency.  PMC
// shows k_compress moves only ~0.4 GB/job — it is latency-bound, so the
// chain length is the lever, not traffic (profiles/pmc_per_launch.json).
__global__ __launch_bounds__(256) void k_compress_ldsin(
    const EmitBlockDesc* __restrict__ bds, uint32_t nblocks,
    const uint8_t* __restrict__ ucblob, uint8_t* __restrict__ cblob,
    uint32_t* __restrict__ bsize, uint8_t* __restrict__ btype) {
  __shared__ uint16_t tabs[4][1u << kSnapHashBits]; // 4 KiB per wave
  __shared__ uint8_t ins[4][5376];
  uint32_t wid = threadIdx.x / WAVE;
  uint32_t lane = threadIdx.x % WAVE;
  uint32_t waves = blockDim.x / WAVE;
  uint16_t* tab = tabs[wid];
  for (uint32_t b = blockIdx.x * waves + wid; b < nblocks;
       b += gridDim.x * waves) {
    EmitBlockDesc d = bds[b];
    if (d.unc_size > SNAP_MAX_UNC) continue; // k_compress_large's block
    const uint8_t* gin = ucblob + d.uout;
    uint32_t n = d.unc_size;
    const uint8_t* in = gin;
    if (n <= sizeof(ins[0])) {
      uint8_t* li = ins[wid];
      for (uint32_t t = lane * 16; t < n; t += WAVE * 16) {
        uint32_t chunk = n - t < 16 ? n - t : 16;
        if (chunk == 16) {
          ulong2 v;
          memcpy(&v, gin + t, 16);
          memcpy(li + t, &v, 16);
        } else {
          for (uint32_t x = 0; x < chunk; x++) li[t + x] = gin[t + x];
        }
      }
      in = li;
    }
    {
      uint32_t* tw = (uint32_t*)tab;
      for (uint32_t t = lane; t < (1u << kSnapHashBits) / 2; t += WAVE)
        tw[t] = 0xffffffffu;
    }
    wave_lds_sync();
    for (uint32_t p = lane; p + 4 <= n; p += WAVE) {
      uint32_t h = (load32(in + p) * kSnapHashMul) >> (32 - kSnapHashBits);
      lds_min_u16(tab, h, p);
    }
    wave_lds_sync();
    uint32_t seg = (uint32_t)snap_segment_size(n);
    uint32_t s0 = lane * seg;
    uint8_t frag[SNAP_FRAG_MAX];
    uint32_t fl = 0;
    if (s0 < n) {
      uint32_t s1 = s0 + seg < n ? s0 + seg : n;
      uint8_t* e = snap_encode_segment_dev(in, s0, s1, tab, frag);
      fl = (uint32_t)(e - frag);
    }
    uint32_t inc = fl;
    for (int sh = 1; sh < WAVE; sh <<= 1) {
      uint32_t v = __shfl_up(inc, sh);
      if ((int)lane >= sh) inc += v;
    }
    uint32_t total = __shfl(inc, WAVE - 1);
    uint32_t excl = inc - fl;
    uint8_t* gout = cblob + d.cout;
    uint8_t hdr[5];
    uint32_t hl = varint32_put(hdr, n);
    if (lane == 0)
      for (uint32_t t = 0; t < hl; t++) gout[t] = hdr[t];
    {
      uint8_t* o2 = gout + hl + excl;
      uint32_t t = 0;
      for (; t + 4 <= fl; t += 4) {
        uint32_t v;
        memcpy(&v, frag + t, 4);
        memcpy(o2 + t, &v, 4);
      }
      for (; t < fl; t++) o2[t] = frag[t];
    }
    if (lane == 0) {
      uint32_t cn = hl + total;
      if (cn <= (((uint64_t)896 * n) >> 10)) {
        bsize[b] = cn;
        btype[b] = 1;
      } else {
        bsize[b] = n;
        btype[b] = 0;
      }
    }
    wave_lds_sync();
  }
}

#define SNAP_LDSIN_MAX 5376 // LDS-staged input bound (default 4 KiB blocks)
template <int LDSIN>
__global__ __launch_bounds__(256, 8) void k_compress_2p(
    const EmitBlockDesc* __restrict__ bds, uint32_t nblocks,
    const uint8_t* __restrict__ ucblob, uint8_t* __restrict__ cblob,
    uint32_t* __restrict__ bsize, uint8_t* __restrict__ btype) {
  __shared__ uint16_t tabs[4][1u << kSnapHashBits]; // 4 KiB per wave
  __shared__ uint8_t ins[LDSIN ? 4 : 1][LDSIN ? SNAP_LDSIN_MAX : 4];
  uint32_t wid = threadIdx.x / WAVE;
  uint32_t lane = threadIdx.x % WAVE;
  uint32_t waves = blockDim.x / WAVE;
  uint16_t* tab = tabs[wid];
  for (uint32_t b = blockIdx.x * waves + wid; b < nblocks;
       b += gridDim.x * waves) {
    EmitBlockDesc d = bds[b];
    if (d.unc_size > SNAP_MAX_UNC) continue; // k_compress_large's block
    const uint8_t* gin = ucblob + d.uout;
    uint32_t n = d.unc_size;
    const uint8_t* in = gin;
    if (LDSIN && n <= SNAP_LDSIN_MAX) {
      uint8_t* li = ins[wid];
      for (uint32_t t = lane * 16; t < n; t += WAVE * 16) {
        uint32_t chunk = n - t < 16 ? n - t : 16;
        if (chunk == 16) {
          ulong2 v;
          memcpy(&v, gin + t, 16);
          memcpy(li + t, &v, 16);
        } else {
          for (uint32_t x = 0; x < chunk; x++) li[t + x] = gin[t + x];
        }
      }
      in = li;
    }
    {
      uint32_t* tw = (uint32_t*)tab;
      for (uint32_t t = lane; t < (1u << kSnapHashBits) / 2; t += WAVE)
        tw[t] = 0xffffffffu;
    }
    wave_lds_sync();
    for (uint32_t p = lane; p + 4 <= n; p += WAVE) {
      uint32_t h = (load32(in + p) * kSnapHashMul) >> (32 - kSnapHashBits);
      lds_min_u16(tab, h, p);
    }
    wave_lds_sync();
    uint32_t seg = (uint32_t)snap_segment_size(n);
    uint32_t s0 = lane * seg;
    uint32_t s1 = s0 + seg < n ? s0 + seg : n;
    uint32_t fl = s0 < n ? snap_measure_segment_dev(in, s0, s1, tab) : 0;
    uint32_t inc = fl;
    for (int sh = 1; sh < WAVE; sh <<= 1) {
      uint32_t v = __shfl_up(inc, sh);
      if ((int)lane >= sh) inc += v;
    }
    uint32_t total = __shfl(inc, WAVE - 1);
    uint32_t excl = inc - fl;
    uint8_t hdr[5];
    uint32_t hl = varint32_put(hdr, n); // lane-uniform
    uint32_t cn = hl + total;
    // GoodCompressionRatio check BEFORE emitting: incompressible blocks
    // write nothing (pack copies the raw block)
    if (cn <= (((uint64_t)896 * n) >> 10)) {
      uint8_t* gout = cblob + d.cout;
      if (lane == 0) {
        for (uint32_t t = 0; t < hl; t++) gout[t] = hdr[t];
        bsize[b] = cn;
        btype[b] = 1;
      }
      if (s0 < n) (void)snap_encode_segment_dev(in, s0, s1, tab, gout + hl + excl);
    } else if (lane == 0) {
      bsize[b] = n;
      btype[b] = 0;
    }
    wave_lds_sync();
  }
}

// ---- large blocks: unc_size > SNAP_MAX_UNC ----
// Same structure as k_compress — one wave per block, all 64 lanes build the
// first-occurrence table, lane i owns segment i — for blocks of any size
// below 2^31.  `big` lists the block indices (the host knows every
// unc_size from the plan).  What changes against the default kernel:
//   - u32 positions (8 KiB of LDS per wave) under plain LDS atomicMin:
//     positions pass 0xffff at n = 65539
//   - no per-lane fragment buffer, a segment is n/64 bytes: two passes as
//     in k_compress_2p.  Pass 1 measures, a shfl prefix sum places the
//     fragments, the ratio test runs on the measured size, and only an
//     accepted block runs pass 2, which writes straight to the slot.  A
//     rejected block writes nothing and is stored raw.
//   - the general measure/emit pair of dcw_snap_enc_big.h (long literal
//     headers, 4-byte-offset copies)
// Writes stay inside the slot: pass 2 runs only when hl + total <=
// (896*n) >> 10 < n, and the slot holds snappy_max_compressed(n) > n bytes.
// n >= 2^31 is refused (DE_BLOCK_PARSE): the 32-bit prefix sums and
// snappy_max_compressed would wrap.
#define SNAP_LARGE_MAX_UNC 0x7fffffffu
__global__ __launch_bounds__(256) void k_compress_large(
    const EmitBlockDesc* __restrict__ bds, const uint32_t* __restrict__ big,
    uint32_t nbig, const uint8_t* __restrict__ ucblob,
    uint8_t* __restrict__ cblob, uint32_t* __restrict__ bsize,
    uint8_t* __restrict__ btype, uint32_t* err_flag) {
  __shared__ uint32_t tabs[4][1u << kSnapHashBits]; // 8 KiB per wave
  uint32_t wid = threadIdx.x / WAVE;
  uint32_t lane = threadIdx.x % WAVE;
  uint32_t waves = blockDim.x / WAVE;
  uint32_t* tab = tabs[wid];
  for (uint32_t i = blockIdx.x * waves + wid; i < nbig;
       i += gridDim.x * waves) {
    uint32_t b = big[i];
    EmitBlockDesc d = bds[b];
    uint32_t n = d.unc_size;
    if (n > SNAP_LARGE_MAX_UNC) {
      if (lane == 0) {
        set_err(err_flag, DE_BLOCK_PARSE);
        bsize[b] = n;
        btype[b] = 0;
      }
      continue;
    }
    const uint8_t* gin = ucblob + d.uout;
    for (uint32_t t = lane; t < (1u << kSnapHashBits); t += WAVE)
      tab[t] = 0xffffffffu;
    wave_lds_sync();
    for (uint32_t p = lane; p + 4 <= n; p += WAVE) {
      uint32_t h = (load32(gin + p) * kSnapHashMul) >> (32 - kSnapHashBits);
      atomicMin(&tab[h], p);
    }
    wave_lds_sync();
    uint32_t seg = (uint32_t)snap_segment_size(n); // <= 2^25: lane*seg fits
    uint32_t s0 = lane * seg;
    uint32_t s1 = s0 + seg < n ? s0 + seg : n;
    uint32_t fl =
        s0 < n ? snapb_walk_segment<false>(gin, s0, s1, tab, nullptr) : 0;
    uint32_t inc = fl;
    for (int sh = 1; sh < WAVE; sh <<= 1) {
      uint32_t v = __shfl_up(inc, sh);
      if ((int)lane >= sh) inc += v;
    }
    uint32_t total = __shfl(inc, WAVE - 1);
    uint32_t excl = inc - fl;
    uint8_t hdr[5];
    uint32_t hl = varint32_put(hdr, n); // lane-uniform
    uint64_t cn = (uint64_t)hl + total;
    // GoodCompressionRatio before any store, as in k_compress_2p
    if (cn <= (((uint64_t)896 * n) >> 10)) {
      uint8_t* gout = cblob + d.cout;
      if (lane == 0) {
        for (uint32_t t = 0; t < hl; t++) gout[t] = hdr[t];
        bsize[b] = (uint32_t)cn;
        btype[b] = 1;
      }
      if (s0 < n)
        (void)snapb_walk_segment<true>(gin, s0, s1, tab, gout + hl + excl);
    } else if (lane == 0) {
      bsize[b] = n;
      btype[b] = 0;
    }
    wave_lds_sync();
  }
}

__global__ void k_checksum(const EmitBlockDesc* __restrict__ bds, uint32_t nblocks,
                           const uint8_t* __restrict__ ucblob,
                           const uint8_t* __restrict__ cblob,
                           const uint32_t* __restrict__ bsize,
                           const uint8_t* __restrict__ btype,
                           uint32_t checksum_type,
                           const Crc32cTables* __restrict__ crc_tt,
                           uint32_t* __restrict__ csum) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < nblocks;
       b += gridDim.x * blockDim.x) {
    const uint8_t* body =
        btype[b] ? cblob + bds[b].cout : ucblob + bds[b].uout;
    csum[b] = block_checksum(checksum_type, crc_tt, body, bsize[b], btype[b]);
  }
}

// pack [body|trailer]* into a contiguous image at host-provided offsets
__global__ void k_pack(const EmitBlockDesc* __restrict__ bds, uint32_t b0,
                       uint32_t b1, const uint8_t* __restrict__ ucblob,
                       const uint8_t* __restrict__ cblob,
                       const uint32_t* __restrict__ bsize,
                       const uint8_t* __restrict__ btype,
                       const uint32_t* __restrict__ csum,
                       const uint64_t* __restrict__ outoff,
                       uint8_t* __restrict__ out) {
  uint32_t waves_per_wg = blockDim.x / WAVE;
  uint32_t wave = blockIdx.x * waves_per_wg + threadIdx.x / WAVE;
  uint32_t lane = threadIdx.x % WAVE;
  for (uint32_t b = b0 + wave; b < b1; b += gridDim.x * waves_per_wg) {
    const uint8_t* body = btype[b] ? cblob + bds[b].cout : ucblob + bds[b].uout;
    uint8_t* dst = out + outoff[b - b0];
    uint32_t n = bsize[b];
    for (uint32_t posn = lane * 16; posn < n; posn += WAVE * 16) {
      uint32_t chunk = n - posn < 16 ? n - posn : 16;
      for (uint32_t t = 0; t < chunk; t++) dst[posn + t] = body[posn + t];
    }
    if (lane == 0) {
      dst[n] = btype[b];
      uint32_t cs = csum[b];
      memcpy(dst + n + 1, &cs, 4);
    }
  }
}

// per-block metadata record, fetched once per chunk together with the
// compressed sizes: boundary keys (for index separators) + seq-range and
// tombstone count (for file properties; replaces a per-file reduce pass)
#define BLKSTAT_STRIDE 160
// record layout (BLKSTAT_STRIDE=160): [klen_f u8 | first ikey <= 56 B at 1]
// [klen_l u8 at 64 | last ikey at 65] [minseq u64 at 128 | maxseq at 136 |
// n_tombstones at 144]
__global__ void k_block_stats(const EmitBlockDesc* __restrict__ bds, uint32_t b0,
                              uint32_t b1, const uint64_t* __restrict__ s_k0,
                              const uint64_t* __restrict__ s_k1,
                              const uint64_t* __restrict__ s_tag,
                              const uint8_t* __restrict__ s_klen,
                              const uint8_t* __restrict__ kext,
                              const uint32_t* __restrict__ s_w,
                              uint8_t* __restrict__ out) {
  for (uint32_t b = b0 + blockIdx.x * blockDim.x + threadIdx.x; b < b1;
       b += gridDim.x * blockDim.x) {
    uint8_t* o = out + (uint64_t)(b - b0) * BLKSTAT_STRIDE;
    uint32_t f = bds[b].first, l = bds[b].first + bds[b].count - 1;
    memset(o, 0, 128);
    o[0] = s_klen[f];
    load_ikey(s_k0[f], s_k1[f], s_tag[f], s_klen[f], kext, s_w, f, o + 1);
    o[64] = s_klen[l];
    load_ikey(s_k0[l], s_k1[l], s_tag[l], s_klen[l], kext, s_w, l, o + 65);
    uint64_t mn = ~0ull, mx = 0, tomb = 0;
    for (uint32_t i = f; i <= l; i++) {
      uint64_t tag = s_tag[i];
      uint64_t seq = tag >> 8;
      if (seq < mn) mn = seq;
      if (seq > mx) mx = seq;
      uint8_t vt = (uint8_t)tag;
      if (vt == kTypeDeletion || vt == kTypeSingleDeletion) tomb++;
    }
    memcpy(o + 128, &mn, 8);
    memcpy(o + 136, &mx, 8);
    memcpy(o + 144, &tomb, 8);
  }
}

// pack survivor range into [klen u8 | key | vlen u32 | value]* records
__global__ void k_gather_range(const uint64_t* __restrict__ s_k0,
                               const uint64_t* __restrict__ s_k1,
                               const uint64_t* __restrict__ s_tag,
                               const uint64_t* __restrict__ s_voff,
                               const uint32_t* __restrict__ s_vlen,
                               const uint8_t* __restrict__ s_klen,
                               const uint8_t* __restrict__ ublob, uint64_t first,
                               uint32_t count, const uint64_t* __restrict__ recoff,
                               const uint8_t* __restrict__ kext,
                               const uint32_t* __restrict__ s_w,
                               uint8_t* __restrict__ out) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += gridDim.x * blockDim.x) {
    uint64_t idx = first + i;
    uint8_t* p = out + recoff[i];
    uint32_t klen = s_klen[idx];
    p[0] = (uint8_t)klen;
    load_ikey(s_k0[idx], s_k1[idx], s_tag[idx], klen, kext, s_w, idx, p + 1);
    uint32_t vl = s_vlen[idx];
    memcpy(p + 1 + klen, &vl, 4);
    const uint8_t* src = ublob + s_voff[idx];
    for (uint32_t t = 0; t < vl; t++) p[5 + klen + t] = src[t];
  }
}

// Per-survivor block planning: for every survivor e, simulate the
// BlockBuilder flush-policy FSM (flush_block_policy.cc:37-52 +
// block_builder.cc estimate accounting) for a block STARTING at e, and
// record where the next block would start plus the block's size/restarts.
// The host then walks the chain from any position — block boundaries after
// a file cut come for free (every entry is a potential block start).
__global__ void k_plan_next(const uint8_t* __restrict__ s_shared,
                            const uint8_t* __restrict__ s_klen,
                            const uint32_t* __restrict__ s_vlen, uint64_t n,
                            uint32_t block_size, uint32_t restart_interval,
                            uint64_t dev_limit, uint32_t* __restrict__ next_out,
                            uint32_t* __restrict__ unc_out,
                            uint16_t* __restrict__ nr_out, uint32_t* err_flag) {
  for (uint64_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t i = e;
    uint64_t bytes = 0;
    uint32_t nrestarts = 1, counter = 0;
    while (i < n) {
      uint32_t klen = s_klen[i], vlen = s_vlen[i];
      uint64_t curr = 8 + bytes + 4 * (nrestarts - 1);
      if (bytes > 0) {
        if (curr >= block_size) break;
        uint64_t after = curr + klen + vlen + 4 + varint_len(klen) +
                         varint_len(vlen) +
                         (counter >= restart_interval ? 4 : 0);
        if (after > block_size && curr > dev_limit && dev_limit != 0) break;
      }
      uint32_t shared = s_shared[i];
      if (counter >= restart_interval) {
        nrestarts++;
        counter = 0;
        shared = 0;
      } else if (bytes == 0) {
        shared = 0;
      }
      uint32_t non_shared = klen - shared;
      bytes += varint_len(shared) + varint_len(non_shared) + varint_len(vlen) +
               non_shared + vlen;
      counter++;
      i++;
    }
    next_out[e] = (uint32_t)i;
    unc_out[e] = (uint32_t)(bytes + 4 * nrestarts + 4);
    nr_out[e] = (uint16_t)nrestarts;
    // unplannable shapes fail the JOB here (DB falls back local) instead of
    // corrupting later: a block k_emit cannot hold, or a restart count that
    // overflows u16 (blocks are <= block_size + one entry; EMIT_MAX_ENTRIES
    // bounds restarts well under 64k for every emit-able block)
    if (i - e > EMIT_MAX_ENTRIES || nrestarts > 0xffffu)
      set_err(err_flag, DE_PLAN_WIDTH);
  }
}

// Grandparent boundary positions (CompactionOutputs::
// UpdateGrandparentBoundaryInfo, compaction_outputs.cc:121-230, recast as a
// pure per-key function): for survivor user key u,
//   A(u) = #files with smallest <= u           (enter transitions)
//   B(u) = #files the walk has fully left:
//          #{i: largest_i < u} + the prefix of the equal-largest run at u
//          whose tie_next flag is set (tie_next_i = smallest_{i+1} ==
//          largest_i, the multi-file same-user-key case, :157-166)
//   pos(u) = A(u)+B(u); odd pos = inside file B(u); nback(u) = #files j <
//   B(u) with largest_j == u (GetCurrentKeyGrandparentOverlappedBytes's
//   backward tie loop, :218-227).
// Every compare is raw bytewise order (bound_cmp): a grandparent key may
// be shorter or longer than the job's uniform `ulen`-byte keys, so its true
// length (gsmlen/glglen) breaks a tie of the padded words.
// The host file-cut FSM consumes pos/nback per survivor.
__global__ void k_gp_positions(const uint64_t* __restrict__ s_k0,
                               const uint64_t* __restrict__ s_k1, uint64_t n,
                               uint32_t ulen,
                               const uint64_t* __restrict__ gsm0,
                               const uint64_t* __restrict__ gsm1,
                               const uint32_t* __restrict__ gsmlen,
                               const uint64_t* __restrict__ glg0,
                               const uint64_t* __restrict__ glg1,
                               const uint32_t* __restrict__ glglen,
                               const uint8_t* __restrict__ tie_next,
                               uint32_t ng, uint32_t* __restrict__ pos_out,
                               uint8_t* __restrict__ nback_out) {
  for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t k0 = s_k0[i], k1 = s_k1[i];
    // A = upper_bound over smallest (count sm <= u)
    uint32_t lo = 0, hi = ng;
    while (lo < hi) {
      uint32_t mid = (lo + hi) / 2;
      bool sm_le = bound_cmp(gsm0[mid], gsm1[mid], gsmlen[mid], nullptr, k0, k1,
                             ulen, nullptr) <= 0;
      if (sm_le)
        lo = mid + 1;
      else
        hi = mid;
    }
    uint32_t A = lo;
    // lb = lower_bound over largest (first lg >= u)
    lo = 0;
    hi = ng;
    while (lo < hi) {
      uint32_t mid = (lo + hi) / 2;
      bool lg_lt = bound_cmp(glg0[mid], glg1[mid], glglen[mid], nullptr, k0, k1,
                             ulen, nullptr) < 0;
      if (lg_lt)
        lo = mid + 1;
      else
        hi = mid;
    }
    uint32_t B = lo;
    uint32_t lb = lo;
    while (B < ng && glg0[B] == k0 && glg1[B] == k1 && glglen[B] == ulen &&
           tie_next[B])
      B++;
    uint32_t nb = 0;
    if (B > lb && glg0[lb] == k0 && glg1[lb] == k1 && glglen[lb] == ulen)
      nb = B - lb;
    pos_out[i] = A + B;
    nback_out[i] = (uint8_t)(nb > 255 ? 255 : nb);
  }
}

__global__ void k_build_headidx(const uint8_t* __restrict__ head,
                                const uint32_t* __restrict__ pos, uint64_t n,
                                uint64_t* __restrict__ headidx) {
  for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x)
    if (head[i]) headidx[pos[i]] = i;
}

__global__ void k_sizes_nocomp(const EmitBlockDesc* __restrict__ bds, uint32_t nb,
                               uint32_t* __restrict__ bsize,
                               uint8_t* __restrict__ btype) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < nb;
       b += gridDim.x * blockDim.x) {
    bsize[b] = bds[b].unc_size;
    btype[b] = 0;
  }
}

__global__ void k_seq_minmax(const uint64_t* __restrict__ s_tag, uint64_t first,
                             uint64_t count, unsigned long long* mn,
                             unsigned long long* mx,
                             unsigned long long* n_tombstones) {
  __shared__ unsigned long long lmn, lmx, ltomb;
  if (threadIdx.x == 0) {
    lmn = ~0ull;
    lmx = 0;
    ltomb = 0;
  }
  __syncthreads();
  unsigned long long tmn = ~0ull, tmx = 0, ttomb = 0;
  for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t tag = s_tag[first + i];
    unsigned long long seq = tag >> 8;
    if (seq < tmn) tmn = seq;
    if (seq > tmx) tmx = seq;
    uint8_t vt = (uint8_t)tag;
    if (vt == kTypeDeletion || vt == kTypeSingleDeletion) ttomb++;
  }
  atomicMin(&lmn, tmn);
  atomicMax(&lmx, tmx);
  atomicAdd(&ltomb, ttomb);
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicMin(mn, lmn);
    atomicMax(mx, lmx);
    if (ltomb) atomicAdd(n_tombstones, ltomb);
  }
}

} // namespace dcw
