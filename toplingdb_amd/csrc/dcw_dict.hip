// dcw_dict.hip — the kernels for input files with a preset dictionary
// ("rocksdb.compression_dict"), and their launchers: k_zstd_dict_prepare and
// the dictionary variants of k_decompress_zstd, k_decompress_zstd_large and
// k_decompress_lz4.  A GPU translation unit of its own, compiled like
// dcw_zstd_large.hip with packed FP32 instructions switched off (Makefile); a
// job without dictionary files launches none of it, and the kernels it does
// launch are built as before.
//
// The format code is shared: the zstd variants are instantiations of
// zstd_dec_frame() with the policies of dcw_zstd_dict.h, the LZ4 variant
// passes an Lz4Dict to the decoders of dcw_lz4_dec.h.  A variant decodes a
// whole work list of a job that has dictionary files, also the list's blocks
// from files without one (slot kNoDict): one launch per kernel per job.  The
// dictionary itself is never staged in LDS: all blocks of a file share it, so
// it stays in L2, and only matches that reach before a block's first byte
// read it.
#include <hip/hip_runtime.h>

#define DCW_ZSTD_WAVE
#include "dcw_lz4_dec.h"
#include "dcw_zstd_dict.h"

namespace dcw {

// s[0, n) in global memory <-> an LDS array d, 16 bytes per lane per step (the
// LDS side aligned), the last n % 16 bytes one per lane
__device__ __forceinline__ void wave_copy16(uint8_t* d, const uint8_t* s, uint32_t n,
                                            uint32_t lane) {
  for (uint32_t t = lane * 16; t + 16 <= n; t += 64 * 16) {
    ulong2 v;
    memcpy(&v, s + t, 16);
    memcpy(d + t, &v, 16);
  }
  const uint32_t t = (n & ~15u) + lane;
  if (lane < 16 && t < n) d[t] = s[t];
}
__device__ __forceinline__ uint32_t preamble_bytes(const uint8_t* src) {
  uint32_t hn = 1; // k_verify_usize accepted it: 1..5 bytes
  while (hn < 5 && (src[hn - 1] & 0x80)) hn++;
  return hn;
}

// One wave (one work-group) per entry of `dicts` that a zstd block uses:
// dictionary -> its ZstdDictTables record.  ~20 KiB of LDS as scratch state.
__global__ __launch_bounds__(64) void k_zstd_dict_prepare(
    const uint8_t* __restrict__ blob, const DictDev* __restrict__ dicts,
    uint32_t ndicts, ZstdDictTables* tabs) {
  __shared__ ZstdLargeLds S;
  const uint32_t lane = threadIdx.x;
  for (uint32_t i = blockIdx.x; i < ndicts; i += gridDim.x) {
    const DictDev dd = dicts[i];
    if (dd.tab == kNoDict) continue;
    zstd_dict_prepare(S, blob + dd.off, dd.size, tabs + dd.tab, lane);
    ZW_SYNC();
  }
}

// k_decompress_zstd with a dictionary: the same staging of frame and decoded
// block in the ZstdWave, one wave per work-group.
__global__ __launch_bounds__(64) void k_decompress_zstd_dict(DictDecodeArgs a) {
  __shared__ ZstdWave S;
  const uint32_t lane = threadIdx.x;
  if (lane < 3) S.tpre[lane] = 0; // no predefined table built yet
  ZW_SYNC();
  for (uint32_t li = blockIdx.x; li < a.nlist; li += gridDim.x) {
    const uint32_t i = a.list[li], slot = a.slot[li];
    const uint8_t* src = a.blob + a.boff[i];
    uint8_t* dst = a.ublob + a.uoff[i];
    const uint32_t un = a.usize[i], hn = preamble_bytes(src);
    src += hn;
    const uint32_t n = a.bsize[i] - hn;
    bool ok = n <= kZstdMax && un <= kZstdMax; // the host lists eligible blocks only
    if (ok) {
      const ZstdDictTables* T = nullptr;
      const uint8_t* dict = nullptr;
      if (slot != kNoDict) {
        const DictDev dd = a.dicts[slot];
        T = a.tabs + dd.tab;
        dict = a.blob + dd.off;
      }
      wave_copy16(S.in, src, n, lane);
      ZW_SYNC();
      ok = zstd_dec_wave_dict(S, T, dict, n, un, lane);
      ZW_SYNC();
      if (ok) wave_copy16(dst, S.out, un, lane);
      ZW_SYNC();
    }
    if (!ok && lane == 0) atomicCAS(a.err_flag, 0u, a.err_code);
  }
}

// k_decompress_zstd_large with a dictionary: global to global, the literal
// scratch as there.
__global__ __launch_bounds__(64) void k_decompress_zstd_large_dict(DictDecodeArgs a,
                                                                    uint8_t* litscr) {
  __shared__ ZstdLargeLds S;
  const uint32_t lane = threadIdx.x;
  if (lane < 3) S.tpre[lane] = 0;
  ZW_SYNC();
  for (uint32_t li = blockIdx.x; li < a.nlist; li += gridDim.x) {
    const uint32_t i = a.list[li], slot = a.slot[li];
    const uint8_t* src = a.blob + a.boff[i];
    const uint32_t un = a.usize[i], hn = preamble_bytes(src);
    bool ok = un <= 0x7fffffffu;
    if (ok) {
      const ZstdDictTables* T = nullptr;
      const uint8_t* dict = nullptr;
      if (slot != kNoDict) {
        const DictDev dd = a.dicts[slot];
        T = a.tabs + dd.tab;
        dict = a.blob + dd.off;
      }
      const ZMemGlobal m = {src + hn, a.ublob + a.uoff[i],
                            litscr + (size_t)blockIdx.x * kZLitStride};
      ok = zstd_dec_wave_large_dict(S, m, T, dict, a.bsize[i] - hn, un, lane);
      ZW_SYNC();
    }
    if (!ok && lane == 0) atomicCAS(a.err_flag, 0u, a.err_code);
  }
}

// k_decompress_lz4 with a dictionary: four waves per work-group, a block per
// wave.  Stream and decoded block are staged in LDS for the serial
// register-window decoder of lane 0; a match that starts in the dictionary
// takes those bytes from global memory, everything else stays in LDS.  A block
// beyond kZstdMax (== DEC_MAX) on either side is decoded global to global.
struct Lz4DictLds {
  uint8_t in[kZstdMax + kZstdPad];
  uint8_t out[kZstdMax + kZstdPad];
};
__global__ __launch_bounds__(256) void k_decompress_lz4_dict(DictDecodeArgs a) {
  __shared__ Lz4DictLds lds[4];
  const uint32_t wid = threadIdx.x / 64, lane = threadIdx.x % 64;
  Lz4DictLds& L = lds[wid];
  for (uint32_t li = blockIdx.x * 4 + wid; li < a.nlist; li += gridDim.x * 4) {
    const uint32_t i = a.list[li], slot = a.slot[li];
    const uint8_t* src = a.blob + a.boff[i];
    uint8_t* dst = a.ublob + a.uoff[i];
    const uint32_t un = a.usize[i], hn = preamble_bytes(src);
    src += hn;
    const uint32_t n = a.bsize[i] - hn;
    Lz4Dict dict = {nullptr, 0};
    if (slot != kNoDict) {
      const DictDev dd = a.dicts[slot];
      dict.e = a.blob + dd.off + dd.size;
      dict.n = dd.size < 65535u ? dd.size : 65535u;
    }
    bool ok = true;
    if (n <= kZstdMax && un <= kZstdMax) {
      wave_copy16(L.in, src, n, lane);
      ZW_SYNC();
      if (lane == 0) ok = lz4_dec_lds(L.in, n, L.out, un, dict);
      ZW_SYNC();
      wave_copy16(dst, L.out, un, lane);
      ZW_SYNC();
    } else if (lane == 0) {
      ok = lz4_dec(src, n, dst, un, dict);
    }
    if (!ok) atomicCAS(a.err_flag, 0u, a.err_code);
  }
}

void launch_zstd_dict_prepare(hipStream_t stream, const uint8_t* blob,
                              const DictDev* dicts, uint32_t ndicts,
                              ZstdDictTables* tabs) {
  hipLaunchKernelGGL(k_zstd_dict_prepare, dim3(ndicts < 1024 ? ndicts : 1024),
                     dim3(64), 0, stream, blob, dicts, ndicts, tabs);
}
void launch_decompress_zstd_dict(uint32_t grid, hipStream_t stream,
                                 const DictDecodeArgs& a) {
  hipLaunchKernelGGL(k_decompress_zstd_dict, dim3(grid), dim3(64), 0, stream, a);
}
void launch_decompress_zstd_large_dict(uint32_t grid, hipStream_t stream,
                                       const DictDecodeArgs& a, uint8_t* litscr) {
  hipLaunchKernelGGL(k_decompress_zstd_large_dict, dim3(grid), dim3(64), 0, stream, a,
                     litscr);
}
void launch_decompress_lz4_dict(uint32_t grid, hipStream_t stream,
                                const DictDecodeArgs& a) {
  hipLaunchKernelGGL(k_decompress_lz4_dict, dim3(grid), dim3(256), 0, stream, a);
}

} // namespace dcw
