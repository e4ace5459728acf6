// dcw_zlib_enc.hip — k_compress_zlib and its launcher.  A GPU translation
// unit of its own beside dcw_gpu.hip, as dcw_zlib.hip is on the decode side,
// so that the other kernels are compiled exactly as before.
#include <hip/hip_runtime.h>

#define DCW_DEFLATE_WAVE
#include "dcw_deflate_enc.h"
#include "dcw_gpu.h"

namespace dcw {

// zlib output (codec, phases and the merging of seam words: dcw_deflate_enc.h).
// One wave per block of any size below 2^31, 4 waves per work-group as in
// k_compress_lz4, each with a DeflLds of its own (about 8.4 KiB).  The block
// is taken window by window (16384 bytes; a default block is one window) in
// two sweeps: the first builds every window's code and adds up the exact bit
// count, the ratio test is lane-uniform arithmetic on that sum and a refused
// block stores nothing; the second writes.  A one-window block still holds
// its table and code then, a larger one rebuilds them per window.
// Writes stay inside the slot: the second sweep runs only when the payload
// is at most (896*n) >> 10 < n bytes, the slot holds 5 +
// deflate_max_compressed(n) > n, and no store reaches a byte at or past the
// measured size.
__global__ __launch_bounds__(256) void k_compress_zlib(
    const EmitBlockDesc* __restrict__ bds, uint32_t nblocks,
    const uint8_t* __restrict__ ucblob, uint8_t* __restrict__ cblob,
    uint32_t* __restrict__ bsize, uint8_t* __restrict__ btype,
    uint32_t* err_flag, uint32_t err_code) {
  __shared__ DeflLds lds[4];
  const uint32_t wid = threadIdx.x / 64, lane = threadIdx.x % 64;
  const uint32_t waves = blockDim.x / 64;
  DeflLds& L = lds[wid];
  for (uint32_t b = blockIdx.x * waves + wid; b < nblocks;
       b += gridDim.x * waves) {
    const EmitBlockDesc d = bds[b];
    const uint32_t n = d.unc_size;
    uint32_t cn = 0;
    if (n > kDeflMaxUnc) {
      if (lane == 0) atomicCAS(err_flag, 0u, err_code);
    } else if (n > 0) {
      cn = defl_enc_wave(L, ucblob + d.uout, n, cblob + d.cout, false, lane);
    }
    if (lane == 0) {
      bsize[b] = cn ? cn : n;
      btype[b] = cn ? 2 : 0;
    }
  }
}

void launch_compress_zlib(uint32_t grid, hipStream_t stream,
                          const EmitBlockDesc* bds, uint32_t nblocks,
                          const uint8_t* ucblob, uint8_t* cblob, uint32_t* bsize,
                          uint8_t* btype, uint32_t* err_flag, uint32_t err_code) {
  hipLaunchKernelGGL(k_compress_zlib, dim3(grid), dim3(256), 0, stream, bds,
                     nblocks, ucblob, cblob, bsize, btype, err_flag, err_code);
}

} // namespace dcw
