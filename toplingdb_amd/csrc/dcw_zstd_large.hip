// dcw_zstd_large.hip — k_decompress_zstd_large and its launcher.  A GPU
// translation unit of its own beside dcw_gpu.hip, so that it is compiled
// with packed FP32 instructions switched off (Makefile) without touching how
// the other kernels are built.
#include <hip/hip_runtime.h>

#define DCW_ZSTD_WAVE
#include "dcw_zstd_dec_large.h"

namespace dcw {

// zstd input blocks (type 7) over kZstdMax on either side, which
// zstd_eligible_large() accepted: one wave per block over its own list,
// global to global (dcw_zstd_dec_large.h).  One wave is one work-group with
// ~20 KiB of LDS for tables and batch state, so the LDS admits 8 work-groups
// per compute unit; `litscr` holds kZLitStride bytes per work-group of the
// grid for Huffman literals.  A refused frame puts err_code into *err_flag
// unless an earlier error stands there.
__global__ __launch_bounds__(64) void k_decompress_zstd_large(
    const uint8_t* __restrict__ blob, const uint64_t* __restrict__ boff,
    const uint32_t* __restrict__ bsize, const uint64_t* __restrict__ uoff,
    const uint32_t* __restrict__ usize, const uint32_t* __restrict__ list,
    uint32_t nlist, uint8_t* ublob, uint8_t* litscr, uint32_t* err_flag,
    uint32_t err_code) {
  __shared__ ZstdLargeLds S;
  const uint32_t lane = threadIdx.x;
  if (lane < 3) S.tpre[lane] = 0; // no predefined table built yet
  ZW_SYNC();
  for (uint32_t li = blockIdx.x; li < nlist; li += gridDim.x) {
    uint32_t i = list[li];
    const uint8_t* src = blob + boff[i];
    uint32_t un = usize[i];
    uint32_t hn = 1; // the preamble again (k_verify_usize accepted it)
    while (hn < 5 && (src[hn - 1] & 0x80)) hn++;
    bool ok = un <= 0x7fffffffu; // the host lists eligible blocks only
    if (ok) {
      const ZMemGlobal m = {src + hn, ublob + uoff[i],
                            litscr + (size_t)blockIdx.x * kZLitStride};
      ok = zstd_dec_wave_large(S, m, bsize[i] - hn, un, lane);
      ZW_SYNC();
    }
    if (!ok && lane == 0) atomicCAS(err_flag, 0u, err_code);
  }
}

void launch_decompress_zstd_large(uint32_t grid, hipStream_t stream,
                                  const uint8_t* blob, const uint64_t* boff,
                                  const uint32_t* bsize, const uint64_t* uoff,
                                  const uint32_t* usize, const uint32_t* list,
                                  uint32_t nlist, uint8_t* ublob, uint8_t* litscr,
                                  uint32_t* err_flag, uint32_t err_code) {
  hipLaunchKernelGGL(k_decompress_zstd_large, dim3(grid), dim3(64), 0, stream,
                     blob, boff, bsize, uoff, usize, list, nlist, ublob, litscr,
                     err_flag, err_code);
}

} // namespace dcw
