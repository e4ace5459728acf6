// dcw_k_filter_dzt.h — bloom filter and DcwZipTable (DZT1) build kernels.
// A section of the single GPU translation unit: dcw_gpu.hip includes the
// dcw_k_*.h headers in order, inside one unit, so every kernel is defined
// before the host code that launches it.  Not a stand-alone header.
#pragma once
#include "dcw_dzt_enc.h"

namespace dcw {

// ------------------------------------------------------------------
// bloom filter build: XXPH3 over user keys + FastLocalBloom
// (util/bloom_impl.h:144-223).  Consecutive-equal-hash dedup matches
// XXPH3FilterBitsBuilder::AddKey exactly.
// ------------------------------------------------------------------
__global__ void k_filter_hashes(const uint64_t* __restrict__ s_k0,
                                const uint64_t* __restrict__ s_k1,
                                const uint8_t* __restrict__ s_klen,
                                const uint8_t* __restrict__ kext,
                                const uint32_t* __restrict__ s_w,
                                uint64_t first, uint64_t count,
                                uint64_t* __restrict__ fhash) {
  for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t e = first + i;
    uint8_t key[DCW_GKEY_MAX + 8];
    uint32_t klen = s_klen[e];
    load_ikey(s_k0[e], s_k1[e], 0 /*tag unused*/, klen, kext, s_w, e, key);
    fhash[i] = xxph3_64(key, klen - 8);
  }
}

__global__ void k_filter_bits(const uint64_t* __restrict__ fhash,
                              uint64_t count, uint32_t len, int num_probes,
                              uint32_t* __restrict__ filter_words) {
  for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (uint64_t)gridDim.x * blockDim.x) {
    if (i > 0 && fhash[i] == fhash[i - 1]) continue; // AddKey dedup
    uint32_t h1 = (uint32_t)fhash[i];
    uint32_t h2 = (uint32_t)(fhash[i] >> 32);
    uint32_t line = bloom_fastrange32(h1, len >> 6) << 6; // byte offset
    uint32_t h = h2;
    for (int p = 0; p < num_probes; p++, h *= 0x9e3779b9u) {
      int bitpos = h >> (32 - 9); // within the 512-bit cache line
      // LE u32 word bit (8*byte + bit) == bitpos & 31
      atomicOr(&filter_words[(line << 3 >> 5) + (bitpos >> 5)],
               1u << (bitpos & 31));
    }
  }
}

// ------------------------------------------------------------------
// DcwZipTable ("DZT1") build kernels — the searchable-compressed SST of
// BASELINE configs[3].  Format + parity: oracle/dzt.c header comment.
// ------------------------------------------------------------------
#define DZTK 64
// value bytes of sampled survivors -> fixed 256 B stride (dict build)
__global__ void k_dzt_sample(const uint32_t* __restrict__ idx, uint32_t n,
                             const uint64_t* __restrict__ s_voff,
                             const uint32_t* __restrict__ s_vlen,
                             const uint8_t* __restrict__ ublob,
                             uint8_t* __restrict__ out) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    uint32_t e = idx[i];
    uint32_t take = s_vlen[e] < 256 ? s_vlen[e] : 256;
    const uint8_t* src = ublob + s_voff[e];
    uint8_t* dst = out + (uint64_t)i * 256;
    for (uint32_t t = 0; t < take; t++) dst[t] = src[t];
  }
}

// first-occurrence hash table over the dict (min-position; matches the
// oracle's serial first-wins scan)
__global__ void k_dict_tab(const uint8_t* __restrict__ dict, uint32_t D,
                           uint32_t* __restrict__ tab) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p + 4 <= D;
       p += gridDim.x * blockDim.x) {
    uint32_t h = (load32(dict + p) * kSnapHashMul) >> (32 - kSnapHashBits);
    atomicMin(&tab[h], p);
  }
}

// gather value bytes of each value block into the contiguous staging blob
__global__ void k_dzt_gather(const GpuJob::DztVBlock* __restrict__ vbs,
                             uint32_t nvb,
                             const uint32_t* __restrict__ voff_entry,
                             uint64_t ent_base,
                             const uint64_t* __restrict__ s_voff,
                             const uint32_t* __restrict__ s_vlen,
                             const uint8_t* __restrict__ ublob,
                             uint8_t* __restrict__ vstage) {
  for (uint32_t b = blockIdx.x; b < nvb; b += gridDim.x) {
    GpuJob::DztVBlock v = vbs[b];
    for (uint32_t li = threadIdx.x; li < v.count; li += blockDim.x) {
      uint64_t e = v.first + li;
      uint8_t* dst = vstage + v.stage_off + voff_entry[e - ent_base];
      const uint8_t* src = ublob + s_voff[e];
      uint32_t vl = s_vlen[e];
      uint32_t t = 0;
      for (; t + 4 <= vl; t += 4) {
        uint32_t w;
        memcpy(&w, src + t, 4);
        memcpy(dst + t, &w, 4);
      }
      for (; t < vl; t++) dst[t] = src[t];
    }
  }
}

// dict-snappy per value block, wave-parallel (spec v4 segmentation; the
// segment encoder is the SAME DCW_HD function the oracle restates)
#define DZT_FRAG_MAX 400 // >= ceil(1.4 * 256-byte segment) + headers
__global__ __launch_bounds__(256, 8) void k_dzt_compress(
    const GpuJob::DztVBlock* __restrict__ vbs, uint32_t nvb,
    const uint8_t* __restrict__ vstage, const uint8_t* __restrict__ dict,
    uint32_t D, const uint32_t* __restrict__ dict_tab,
    uint8_t* __restrict__ cblob, uint64_t ccap,
    uint32_t* __restrict__ bsize, uint8_t* __restrict__ btype,
    uint32_t* err_flag) {
  // u16 virtual positions (max 65532 < 0xffff sentinel), same occupancy
  // lift as k_compress: 4 KiB table per wave
  __shared__ uint16_t tabs[4][1u << kSnapHashBits];
  uint32_t wid = threadIdx.x / WAVE;
  uint32_t lane = threadIdx.x % WAVE;
  uint32_t waves = blockDim.x / WAVE;
  uint16_t* tab = tabs[wid];
  for (uint32_t b = blockIdx.x * waves + wid; b < nvb; b += gridDim.x * waves) {
    GpuJob::DztVBlock v = vbs[b];
    uint32_t n = v.ulen;
    if (n > SNAP_MAX_UNC) { // oversize single-value block stays raw
      if (lane == 0) {
        bsize[b] = n;
        btype[b] = 0;
      }
      continue;
    }
    const uint8_t* gin = vstage + v.stage_off;
    for (uint32_t t = lane; t < (1u << kSnapHashBits); t += WAVE) {
      uint32_t dv = dict_tab[t]; // dict positions < D <= 48 KiB fit u16
      tab[t] = (uint16_t)(dv > 0xffffu ? 0xffffu : dv);
    }
    wave_lds_sync();
    for (uint32_t p = lane; p + 4 <= n; p += WAVE) {
      uint32_t h = (load32(gin + p) * kSnapHashMul) >> (32 - kSnapHashBits);
      lds_min_u16(tab, h, D + p); // dict positions (< D) always win
    }
    wave_lds_sync();
    uint32_t seg = (uint32_t)snap_segment_size(n);
    uint32_t s0 = lane * seg;
    // dict copies may use the 5-byte (4-byte-offset) form: worst case is
    // ~1.4 bytes out per segment byte (alternating 1-literal + 4-byte
    // match), so the fragment buffer must exceed SNAP_FRAG_MAX
    uint8_t frag[DZT_FRAG_MAX];
    uint32_t fl = 0;
    if (s0 < n) {
      uint32_t s1 = s0 + seg < n ? s0 + seg : n;
      uint8_t* e = snap_encode_segment_dict(dict, D, gin, D + s0, D + s1, tab,
                                            frag);
      fl = (uint32_t)(e - frag);
    }
    uint32_t inc = fl;
    for (int sh = 1; sh < WAVE; sh <<= 1) {
      uint32_t x = __shfl_up(inc, sh);
      if ((int)lane >= sh) inc += x;
    }
    uint32_t total = __shfl(inc, WAVE - 1);
    uint32_t excl = inc - fl;
    uint8_t* gout = cblob + (uint64_t)b * ccap;
    uint8_t hdr[5];
    uint32_t hl = varint32_put(hdr, n);
    if (lane == 0)
      for (uint32_t t = 0; t < hl; t++) gout[t] = hdr[t];
    {
      uint8_t* o2 = gout + hl + excl;
      uint32_t t = 0;
      for (; t + 4 <= fl; t += 4) {
        uint32_t w;
        memcpy(&w, frag + t, 4);
        memcpy(o2 + t, &w, 4);
      }
      for (; t < fl; t++) o2[t] = frag[t];
    }
    if (lane == 0) {
      uint32_t cn = hl + total;
      if (cn <= (((uint64_t)896 * n) >> 10)) {
        bsize[b] = cn;
        btype[b] = 2; // dict-snappy
      } else {
        bsize[b] = n;
        btype[b] = 0;
      }
    }
    wave_lds_sync();
  }
}

__global__ void k_dzt_checksum(const GpuJob::DztVBlock* __restrict__ vbs,
                               uint32_t nvb, const uint8_t* __restrict__ vstage,
                               const uint8_t* __restrict__ cblob, uint64_t ccap,
                               const uint32_t* __restrict__ bsize,
                               const uint8_t* __restrict__ btype,
                               uint32_t checksum_type,
                               const Crc32cTables* __restrict__ crc_tt,
                               uint32_t* __restrict__ csum) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < nvb;
       b += gridDim.x * blockDim.x) {
    const uint8_t* body =
        btype[b] == 2 ? cblob + (uint64_t)b * ccap : vstage + vbs[b].stage_off;
    csum[b] = block_checksum(checksum_type, crc_tt, body, bsize[b], btype[b]);
  }
}

__global__ void k_dzt_pack(const GpuJob::DztVBlock* __restrict__ vbs,
                           uint32_t nvb, const uint8_t* __restrict__ vstage,
                           const uint8_t* __restrict__ cblob, uint64_t ccap,
                           const uint32_t* __restrict__ bsize,
                           const uint8_t* __restrict__ btype,
                           const uint32_t* __restrict__ csum,
                           const uint64_t* __restrict__ outoff,
                           uint8_t* __restrict__ out) {
  uint32_t waves_per_wg = blockDim.x / WAVE;
  uint32_t wave = blockIdx.x * waves_per_wg + threadIdx.x / WAVE;
  uint32_t lane = threadIdx.x % WAVE;
  for (uint32_t b = wave; b < nvb; b += gridDim.x * waves_per_wg) {
    const uint8_t* body =
        btype[b] == 2 ? cblob + (uint64_t)b * ccap : vstage + vbs[b].stage_off;
    uint8_t* dst = out + outoff[b];
    uint32_t n = bsize[b];
    for (uint32_t pos = lane * 16; pos < n; pos += WAVE * 16) {
      uint32_t chunk = n - pos < 16 ? n - pos : 16;
      for (uint32_t t = 0; t < chunk; t++) dst[pos + t] = body[pos + t];
    }
    if (lane == 0) {
      dst[n] = btype[b];
      uint32_t cs = csum[b];
      memcpy(dst + n + 1, &cs, 4);
    }
  }
}

// key area: one workgroup per key block (record layout per oracle/dzt.c);
// thread 0 also writes the block's first internal key (key index input)
__global__ void k_dzt_keys(const GpuJob::DztKBlock* __restrict__ kbs,
                           uint32_t nkb, const uint64_t* __restrict__ s_k0,
                           const uint64_t* __restrict__ s_k1,
                           const uint64_t* __restrict__ s_tag,
                           const uint8_t* __restrict__ s_klen,
                           const uint8_t* __restrict__ s_sshared,
                           const uint32_t* __restrict__ voff_entry,
                           uint64_t ent_base,
                           const uint32_t* __restrict__ s_vlen,
                           uint32_t ukey_len, uint8_t* __restrict__ keyarea,
                           uint8_t* __restrict__ first_ikeys,
                           uint32_t ik_stride, uint32_t* err_flag) {
  __shared__ uint32_t offs[DZTK];
  __shared__ uint32_t esz[DZTK];
  for (uint32_t kb = blockIdx.x; kb < nkb; kb += gridDim.x) {
    GpuJob::DztKBlock K = kbs[kb];
    if (K.count > DZTK) {
      if (threadIdx.x == 0) set_err(err_flag, DE_BLOCK_PARSE);
      __syncthreads();
      continue;
    }
    for (uint32_t li = threadIdx.x; li < K.count; li += blockDim.x) {
      uint64_t e = K.first + li;
      uint32_t sh = li == 0 ? 0 : s_sshared[e];
      if (sh > ukey_len) sh = ukey_len;
      uint32_t ns = ukey_len - sh;
      esz[li] = varint_len(sh) + varint_len(ns) + ns + 8 + 4 + 4;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t off = 0;
      for (uint32_t li = 0; li < K.count; li++) {
        offs[li] = off;
        off += esz[li];
      }
    }
    __syncthreads();
    for (uint32_t li = threadIdx.x; li < K.count; li += blockDim.x) {
      uint64_t e = K.first + li;
      uint32_t sh = li == 0 ? 0 : s_sshared[e];
      if (sh > ukey_len) sh = ukey_len;
      uint32_t ns = ukey_len - sh;
      uint8_t key[24];
      build_ikey(s_k0[e], s_k1[e], s_tag[e], s_klen[e], key);
      uint8_t* p = keyarea + K.koff + offs[li];
      p += varint32_put(p, sh);
      p += varint32_put(p, ns);
      for (uint32_t t = 0; t < ns; t++) p[t] = key[sh + t];
      p += ns;
      memcpy(p, key + ukey_len, 8); // tag
      p += 8;
      uint32_t vo = voff_entry[e - ent_base];
      memcpy(p, &vo, 4);
      p += 4;
      uint32_t vl = s_vlen[e];
      memcpy(p, &vl, 4);
    }
    if (threadIdx.x == 0) {
      uint8_t key[24];
      build_ikey(s_k0[K.first], s_k1[K.first], s_tag[K.first], s_klen[K.first],
                 key);
      memcpy(first_ikeys + (uint64_t)kb * ik_stride, key, ik_stride);
    }
    __syncthreads();
  }
}

// General-key variant of k_dzt_keys: survivors of one user-key length U in
// 1..DCW_GKEY_MAX whose key bytes live in the side table kext (row s_w[e]).
// One wave per key block, one lane per record: the record offsets come from
// a shuffle scan of the record sizes, and each lane copies its non-shared
// suffix from the side table straight into the record (dcw_dzt_enc.h) — no
// private key buffer, so nothing is indexed at run time in scratch.  Lane 0
// also writes the block's first internal key (U+8 bytes, row stride
// ik_stride).  Launch with blockDim.x == WAVE.
__global__ __launch_bounds__(WAVE) void k_dzt_keys_g(
    const GpuJob::DztKBlock* __restrict__ kbs, uint32_t nkb,
    const uint8_t* __restrict__ kext, const uint32_t* __restrict__ s_w,
    const uint64_t* __restrict__ s_tag, const uint8_t* __restrict__ s_sshared,
    const uint32_t* __restrict__ voff_entry, uint64_t ent_base,
    const uint32_t* __restrict__ s_vlen, uint32_t ukey_len,
    uint8_t* __restrict__ keyarea, uint8_t* __restrict__ first_ikeys,
    uint32_t ik_stride, uint32_t* err_flag) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t kb = blockIdx.x; kb < nkb; kb += gridDim.x) {
    GpuJob::DztKBlock K = kbs[kb];
    if (K.count > DZTK || blockDim.x != WAVE) { // uniform across the wave
      if (lane == 0) set_err(err_flag, DE_BLOCK_PARSE);
      continue;
    }
    const bool act = lane < K.count;
    const uint64_t e = K.first + (act ? lane : 0);
    uint32_t sh = dzt_krec_shared(s_sshared[e], ukey_len, lane == 0);
    uint32_t sz = act ? dzt_krec_size(sh, ukey_len) : 0;
    uint32_t inc = sz;
    for (int d = 1; d < WAVE; d <<= 1) {
      uint32_t x = __shfl_up(inc, d);
      if ((int)lane >= d) inc += x;
    }
    if (act) { // no early continue: the wave meets whole at the next scan
      const uint8_t* ukey = kext + (uint64_t)s_w[e] * DCW_GKEY_STRIDE;
      uint64_t tag = s_tag[e];
      dzt_krec_put(keyarea + K.koff + (inc - sz), sh, ukey_len, ukey, tag,
                   voff_entry[e - ent_base], s_vlen[e]);
      if (lane == 0) {
        uint8_t* fk = first_ikeys + (uint64_t)kb * ik_stride;
        dzt_copy_bytes(fk, ukey, ukey_len);
        store64(fk + ukey_len, tag);
      }
    }
  }
}

} // namespace dcw
