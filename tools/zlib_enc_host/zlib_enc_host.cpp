// zlib_enc_host — the deflate output encoder (dcw_deflate_enc.h, the source
// k_compress_zlib compiles) driven on the CPU without a GPU.  The wave form
// is the kernel's own text: every phase runs as a loop over the 64 lanes,
// here once ascending and once descending, the LDS counters as plain
// integers.  For every block of a corpus file it
//   1. runs defl_enc_wave into a heap buffer of EXACTLY the measured payload
//      size, also where the ratio rule refuses the block: under
//      AddressSanitizer a store past what was measured is a heap overflow,
//      and the input is a heap copy of exactly n bytes;
//   2. requires both lane orders to give the bytes of deflate_encode_block
//      (the serial restatement);
//   3. requires the stream to decode back to the block through inflate_dec.
//
// Build: g++ -fsanitize=address,undefined -I toplingdb_amd/csrc
//            tools/zlib_enc_host/zlib_enc_host.cpp  (tests/test_zlib_output_cpu.py)
//
// usage: zlib_enc_host <corpus file> <streams file>
// Corpus, little-endian: (u32 name length, name, u32 n, n bytes)*
// Streams: (u32 length, stored payload)* in corpus order.
// Prints "block <name> <n> <payload bytes> <accepted>" per block, accepted
// being the worker's ratio test, then "OK".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#define DCW_DEFLATE_WAVE
#include "dcw_deflate_enc.h"
#include "dcw_inflate_dec.h"

using namespace dcw;

namespace {

int fail(const std::string& name, const char* what) {
  printf("FAIL %s: %s\n", name.c_str(), what);
  return 1;
}

int run_block(const std::string& name, const uint8_t* in, uint32_t n,
              std::ofstream& streams) {
  std::vector<uint8_t> ref(5 + deflate_max_compressed(n));
  size_t cn = deflate_encode_block(in, n, ref.data());
  if (cn > ref.size()) return fail(name, "past deflate_max_compressed");
  int accepted = cn <= (((uint64_t)896 * n) >> 10) ? 1 : 0;
  auto lds = std::make_unique<DeflLds>();
  for (dw_descending = 0; dw_descending < 2; dw_descending++) {
    std::unique_ptr<uint8_t[]> out(new uint8_t[cn]);
    memset(out.get(), 0xa5, cn);
    memset(lds.get(), 0x5a, sizeof(DeflLds)); // the wave owes LDS nothing
    if (defl_enc_wave(*lds, in, n, out.get(), true, 0) != cn)
      return fail(name, "wave size != deflate_encode_block");
    if (memcmp(out.get(), ref.data(), cn) != 0)
      return fail(name, "wave bytes != deflate_encode_block");
    if ((defl_enc_wave(*lds, in, n, out.get(), false, 0) != 0) != (accepted != 0))
      return fail(name, "ratio rule");
  }
  dw_descending = 0;
  uint32_t un = 0;
  int hl = zlib_preamble(ref.data(), (uint32_t)cn, &un);
  std::unique_ptr<uint8_t[]> back(new uint8_t[n]);
  if (hl < 0 || un != n ||
      !inflate_dec(ref.data() + hl, (uint32_t)(cn - hl), back.get(), n) ||
      memcmp(back.get(), in, n) != 0)
    return fail(name, "round trip through inflate_dec");
  uint32_t cn32 = (uint32_t)cn;
  streams.write((const char*)&cn32, 4);
  streams.write((const char*)ref.data(), (std::streamsize)cn);
  printf("block %s %u %zu %d\n", name.c_str(), n, cn, accepted);
  return 0;
}

} // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: zlib_enc_host <corpus file> <streams file>\n");
    return 2;
  }
  std::ifstream fs(argv[1], std::ios::binary);
  std::ofstream streams(argv[2], std::ios::binary);
  if (!fs || !streams) {
    fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
    return 2;
  }
  std::string buf((std::istreambuf_iterator<char>(fs)),
                  std::istreambuf_iterator<char>());
  size_t at = 0, blocks = 0;
  while (at < buf.size()) {
    uint32_t nl = 0, n = 0;
    if (buf.size() - at < 4) return fail("corpus", "truncated");
    memcpy(&nl, buf.data() + at, 4);
    at += 4;
    if (buf.size() - at < (size_t)nl + 4) return fail("corpus", "truncated");
    std::string name(buf.data() + at, nl);
    at += nl;
    memcpy(&n, buf.data() + at, 4);
    at += 4;
    if (buf.size() - at < n || n == 0 || n > kDeflMaxUnc)
      return fail(name, "bad block length");
    // a heap copy of exactly n bytes: a read past the block is an overflow
    std::unique_ptr<uint8_t[]> in(new uint8_t[n]);
    memcpy(in.get(), buf.data() + at, n);
    at += n;
    if (run_block(name, in.get(), n, streams) != 0) return 1;
    blocks++;
  }
  if (blocks == 0) return fail("corpus", "empty");
  streams.close();
  if (!streams) return fail("streams", "write failed");
  printf("OK\n");
  return 0;
}
