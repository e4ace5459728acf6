// dcw_k_dzt_in.h — decode-side kernels for DcwZipTable ("DZT1") INPUT
// files: value-block verify, dict-snappy decode, key-block decode.  They
// fill the same entry arrays (ents/voff/vlen/klen/kext) as the
// BlockBasedTable decode kernels, so merge and dedup see no difference.
// A section of the single GPU translation unit (see dcw_k_decode.h); the
// block decoders themselves are the shared plain-C++ ones of dcw_dzt_dec.h.
#pragma once
#include "dcw_dzt_dec.h"
#include "dcw_k_decode.h"

namespace dcw {

// host-built tables (GpuJob::decode), one row per value block / key block /
// file, all DZT files of the job concatenated in run-major file order
struct DztVbIn {
  uint64_t off;  // stored block (body | btype | csum) in the input blob
  uint64_t uoff; // decoded bytes, relative to the DZT part of the ublob
  uint32_t csize, ulen;
  uint32_t first_rank; // file-local rank of the block's first value
  uint32_t file;
};
struct DztKbIn {
  uint64_t off;      // key block in the input blob
  uint64_t kidx_off; // this block's key-index row (first_ikey[U+8] ...)
  uint32_t ksize;
  uint32_t count;      // records, from the index's first_rank differences
  uint32_t first_rank; // file-local
  uint32_t out_base;   // entry position of the block's first record
  uint32_t vb_start;   // value block holding first_rank (row in DztVbIn)
  uint32_t file;
  uint32_t has_next; // another key block of the same file follows
  uint32_t pad;
};
struct DztFileIn {
  uint64_t dict_off; // in the input blob
  uint32_t dict_size;
  uint32_t U;      // uniform user-key length of the file
  uint32_t vb_end; // one past the file's last DztVbIn row
  uint32_t pad;
};

// One thread per stored value block: trailer checksum over body + btype,
// then the length the index promised.  Same trailer shape as a
// BlockBasedTable block, so the same block_checksum.  The host has already
// checked off + csize + 5 against the file's value area.
__global__ void k_dzt_verify_vblocks(const uint8_t* __restrict__ blob,
                                     const DztVbIn* __restrict__ vbs,
                                     uint32_t nvb, uint32_t checksum_type,
                                     const Crc32cTables* __restrict__ crc_tt,
                                     uint8_t* __restrict__ btype,
                                     uint32_t* err_flag) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nvb;
       i += gridDim.x * blockDim.x) {
    const uint8_t* p = blob + vbs[i].off;
    uint32_t sz = vbs[i].csize;
    uint8_t type = p[sz];
    uint32_t stored;
    memcpy(&stored, p + sz + 1, 4);
    if (checksum_type != 0 &&
        block_checksum(checksum_type, crc_tt, p, sz, type) != stored) {
      set_err(err_flag, DE_CHECKSUM);
      return;
    }
    if (type == 0) {
      if (sz != vbs[i].ulen) {
        set_err(err_flag, DE_BLOCK_PARSE);
        return;
      }
    } else if (type == 2) {
      // (size_t)-1 for a bad varint never equals a u32 ulen
      if (snappy_uncompressed_len(p, sz) != (size_t)vbs[i].ulen) {
        set_err(err_flag, DE_SNAPPY);
        return;
      }
    } else {
      set_err(err_flag, DE_COMPRESS_TYPE);
      return;
    }
    btype[i] = type;
  }
}

// Dict-snappy decode, one wave (= one workgroup) per value block, following
// k_decompress: all lanes stage the stream into LDS, lane 0 runs the serial
// decoder LDS -> LDS, all lanes copy the result out.  The dictionary stays
// in global memory: it is read-only and shared by every block of its file,
// and 48 KiB of it per workgroup would leave two or three workgroups per CU.
// LDS per workgroup: 14336 + 16384 = 30720 B -> 5 workgroups (5 decoders)
// per CU of the 160 KiB.  DZT_DEC_OUT is the format's value-block bound;
// DZT_DEC_IN the largest stream the builder keeps ((896 * 16384) >> 10).
// A block over either bound — a single oversize value, or a foreign stream
// that did not shrink — is decoded global -> global by lane 0.
#define DZT_DEC_IN 14336
#define DZT_DEC_OUT 16384
struct DztDecLds {
  uint8_t in[DZT_DEC_IN];
  uint8_t out[DZT_DEC_OUT];
};

__global__ __launch_bounds__(WAVE) void k_dzt_decompress(
    const uint8_t* __restrict__ blob, const DztVbIn* __restrict__ vbs,
    const DztFileIn* __restrict__ files, const uint8_t* __restrict__ btype,
    uint32_t nvb, uint8_t* __restrict__ ublob, uint32_t* err_flag) {
  __shared__ DztDecLds L;
  uint32_t lane = threadIdx.x;
  for (uint32_t i = blockIdx.x; i < nvb; i += gridDim.x) {
    const uint8_t* src = blob + vbs[i].off;
    uint8_t* dst = ublob + vbs[i].uoff;
    uint32_t n = vbs[i].csize, un = vbs[i].ulen;
    const uint8_t* dict = blob + files[vbs[i].file].dict_off;
    uint32_t D = files[vbs[i].file].dict_size;
    if (btype[i] == 0) { // raw: n == un (k_dzt_verify_vblocks)
      for (uint32_t pos = lane * 16; pos + 16 <= n; pos += WAVE * 16) {
        ulong2 v;
        memcpy(&v, src + pos, 16);
        memcpy(dst + pos, &v, 16);
      }
      if (lane == 0)
        for (uint32_t t = n & ~15u; t < n; t++) dst[t] = src[t];
    } else if (n <= DZT_DEC_IN && un <= DZT_DEC_OUT) {
      for (uint32_t t = lane * 16; t + 16 <= n; t += WAVE * 16) {
        ulong2 v;
        memcpy(&v, src + t, 16);
        memcpy(L.in + t, &v, 16);
      }
      if (lane == 0)
        for (uint32_t t = n & ~15u; t < n; t++) L.in[t] = src[t];
      wave_lds_sync2();
      if (lane == 0) {
        uint32_t got = 0;
        if (dzt_snap_dec(dict, D, L.in, n, L.out, un, &got) != DZT_OK ||
            got != un)
          set_err(err_flag, DE_SNAPPY);
      }
      wave_lds_sync2();
      for (uint32_t t = lane * 16; t + 16 <= un; t += WAVE * 16) {
        ulong2 v;
        memcpy(&v, L.out + t, 16);
        memcpy(dst + t, &v, 16);
      }
      if (lane == 0)
        for (uint32_t t = un & ~15u; t < un; t++) dst[t] = L.out[t];
      wave_lds_sync2();
    } else if (lane == 0) {
      uint32_t got = 0;
      if (dzt_snap_dec(dict, D, src, n, dst, un, &got) != DZT_OK || got != un)
        set_err(err_flag, DE_SNAPPY);
    }
  }
}

// One lane per key block: records are prefix-chained inside a block and
// independent across blocks; the index's first_rank gives every output
// position up front, so there is no count pass.  Beyond the per-record
// checks of dzt_key_next: the block holds exactly `count` records in
// exactly ksize bytes; its first key is the one the index names; its last
// key sorts before the next block's first key; every value lies inside its
// value block.  general != 0 also fills the full-key side table.
__global__ void k_dzt_decode_keys(
    const uint8_t* __restrict__ blob, const DztKbIn* __restrict__ kbs,
    uint32_t nkb, const DztVbIn* __restrict__ vbs,
    const DztFileIn* __restrict__ files, uint64_t dzt_ubase, int general,
    ulong4* __restrict__ ents, uint64_t* __restrict__ voff,
    uint32_t* __restrict__ vlen_out, uint8_t* __restrict__ klen_out,
    uint8_t* __restrict__ kext, uint32_t* err_flag) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nkb;
       i += gridDim.x * blockDim.x) {
    const DztKbIn K = kbs[i];
    const uint32_t U = files[K.file].U, vb_end = files[K.file].vb_end;
    const uint8_t* kb = blob + K.off;
    const uint8_t* kidx = blob + K.kidx_off;
    uint8_t key[kDztUkeyMax];
    for (uint32_t t = 0; t < kDztUkeyMax; t++) key[t] = 0;
    uint32_t pos = 0, vb = K.vb_start;
    uint64_t prev_tag = 0;
    for (uint32_t j = 0; j < K.count; j++) {
      DztKeyRec r;
      int rc = pos < K.ksize ? dzt_key_next(kb, K.ksize, &pos, U, j == 0, key,
                                            prev_tag, &r)
                             : (int)DZT_E_BLOCK_PARSE;
      if (rc != DZT_OK) {
        set_err(err_flag, (uint32_t)rc);
        return;
      }
      prev_tag = r.tag;
      if (j == 0) { // the index must name this block's first internal key
        bool same = load64(kidx + U) == r.tag;
        for (uint32_t t = 0; t < U; t++) same = same && kidx[t] == key[t];
        if (!same) {
          set_err(err_flag, DE_BLOCK_PARSE);
          return;
        }
      }
      uint32_t rank = K.first_rank + j;
      while (vb + 1 < vb_end && vbs[vb + 1].first_rank <= rank) vb++;
      if ((uint64_t)r.voff + r.vlen > vbs[vb].ulen) {
        set_err(err_flag, DE_BLOCK_PARSE);
        return;
      }
      uint64_t out = (uint64_t)K.out_base + j;
      uint64_t u0 = 0, u1 = 0;
      for (uint32_t t = 0; t < U && t < 8; t++)
        u0 |= (uint64_t)key[t] << (8 * t);
      for (uint32_t t = 8; t < U && t < 16; t++)
        u1 |= (uint64_t)key[t] << (8 * (t - 8));
      ents[out] = make_ulong4(__builtin_bswap64(u0), __builtin_bswap64(u1),
                              ~r.tag, out);
      if (general) {
        uint8_t* slot = kext + out * (uint64_t)DCW_GKEY_STRIDE;
        for (uint32_t t = 0; t < U; t++) slot[t] = key[t];
        for (uint32_t t = U; t < DCW_GKEY_STRIDE; t++) slot[t] = 0;
      }
      voff[out] = dzt_ubase + vbs[vb].uoff + r.voff;
      vlen_out[out] = r.vlen;
      klen_out[out] = (uint8_t)(U + 8);
    }
    if (pos != K.ksize) { // a 65th record, or bytes no record owns
      set_err(err_flag, DE_BLOCK_PARSE);
      return;
    }
    if (K.has_next && K.count) {
      const uint8_t* nk = kidx + (U + 28); // next row's first_ikey
      int cmp = 0;
      for (uint32_t t = 0; t < U && cmp == 0; t++)
        if (key[t] != nk[t]) cmp = key[t] < nk[t] ? -1 : 1;
      if (cmp > 0 || (cmp == 0 && prev_tag <= load64(nk + U))) {
        set_err(err_flag, DE_BLOCK_PARSE);
        return;
      }
    }
  }
}

} // namespace dcw
