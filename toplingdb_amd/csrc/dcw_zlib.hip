// dcw_zlib.hip — k_decompress_zlib and its launcher.  A GPU translation unit
// of its own beside dcw_gpu.hip, as dcw_zstd_large.hip and dcw_dict.hip are,
// so that the other kernels are compiled exactly as before.
#include <hip/hip_runtime.h>

#define DCW_INFLATE_WAVE
#include "dcw_inflate_dec.h"

namespace dcw {

// What one wave owns: the decoder's tables and batch state, and the staging
// of a block whose stream and decoded size are both within kInflMax.
struct alignas(16) InflWave {
  InflLds t;
  alignas(16) uint8_t in[kInflMax];
  alignas(16) uint8_t out[kInflMax];
};

// zlib input blocks (type 2), one wave per block over the host-built list of
// their indices; one wave is one work-group, as for k_decompress_zstd.  A
// block within kInflMax on both sides is staged in LDS with 16-byte
// cooperative copies and decoded there (InflMemLds); any other block is
// decoded from the staged blob straight into its slot of the decoded blob
// (InflMemGlobal), its matches reading back what the wave stored.  A refused
// stream puts err_code into *err_flag unless an earlier error stands there;
// it stores nothing outside the block's own slot.
__global__ __launch_bounds__(64) void k_decompress_zlib(
    const uint8_t* __restrict__ blob, const uint64_t* __restrict__ boff,
    const uint32_t* __restrict__ bsize, const uint64_t* __restrict__ uoff,
    const uint32_t* __restrict__ usize, const uint32_t* __restrict__ list,
    uint32_t nlist, uint8_t* ublob, uint32_t* err_flag, uint32_t err_code) {
  __shared__ InflWave W;
  const uint32_t lane = threadIdx.x;
  if (lane == 0) W.t.tfixed = 0; // the fixed code's tables are not built yet
  IW_SYNC();
  for (uint32_t li = blockIdx.x; li < nlist; li += gridDim.x) {
    const uint32_t i = list[li];
    const uint8_t* src = blob + boff[i];
    uint8_t* dst = ublob + uoff[i];
    const uint32_t un = usize[i];
    uint32_t hn = 1; // the preamble again (k_verify_usize accepted it)
    while (hn < 5 && (src[hn - 1] & 0x80)) hn++;
    src += hn;
    const uint32_t n = bsize[i] - hn;
    bool ok;
    if (n <= kInflMax && un <= kInflMax) {
      // the stream starts behind the preamble, so the loads are unaligned
      // global loads; the LDS side of every copy is aligned
      for (uint32_t t = lane * 16; t + 16 <= n; t += 64 * 16) {
        ulong2 v;
        memcpy(&v, src + t, 16);
        memcpy(W.in + t, &v, 16);
      }
      if (lane == 0)
        for (uint32_t t = n & ~15u; t < n; t++) W.in[t] = src[t];
      IW_SYNC();
      const InflMemLds m = {W.in, W.out};
      ok = infl_dec_wave(W.t, m, n, un, lane);
      IW_SYNC();
      if (ok) {
        for (uint32_t t = lane * 16; t + 16 <= un; t += 64 * 16) {
          ulong2 v;
          memcpy(&v, W.out + t, 16);
          memcpy(dst + t, &v, 16);
        }
        if (lane == 0)
          for (uint32_t t = un & ~15u; t < un; t++) dst[t] = W.out[t];
      }
      IW_SYNC();
    } else {
      const InflMemGlobal m = {src, dst};
      ok = infl_dec_wave(W.t, m, n, un, lane);
      IW_SYNC();
    }
    if (!ok && lane == 0) atomicCAS(err_flag, 0u, err_code);
  }
}

void launch_decompress_zlib(uint32_t grid, hipStream_t stream, const uint8_t* blob,
                            const uint64_t* boff, const uint32_t* bsize,
                            const uint64_t* uoff, const uint32_t* usize,
                            const uint32_t* list, uint32_t nlist, uint8_t* ublob,
                            uint32_t* err_flag, uint32_t err_code) {
  hipLaunchKernelGGL(k_decompress_zlib, dim3(grid), dim3(64), 0, stream, blob,
                     boff, bsize, uoff, usize, list, nlist, ublob, err_flag,
                     err_code);
}

} // namespace dcw
