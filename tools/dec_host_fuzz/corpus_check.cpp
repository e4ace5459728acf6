// Runs a file of snappy streams through the host-compiled snap_dec_lds
// (PIPE=0 and PIPE=1, from the kernels' own header) and the snap_dec_wave
// simulation, and compares with the expected bytes.  The streams come from
// encoders other than the project's own (tests/foreign_snappy.py), so the
// decoders meet op forms its codec never emits before any GPU time is spent.
//
//   corpus_check <file>
// file: records of  u32 n | u32 rawlen | n stream bytes | rawlen raw bytes;
// rawlen == 0xffffffff marks a malformed stream every decoder must refuse
// (no raw bytes follow).
#include <cstdint>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __device__
#define __forceinline__ inline
#include "dcw_snap_dec_lds.h"
#include "dec_host.h"
#include "wave_sim.h"

typedef uint32_t (*dec_fn)(const uint8_t*, uint32_t, uint8_t*, uint32_t);
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  const dec_fn decs[3] = {snap_dec_lds_host0, snap_dec_lds_host, dec_wave_sim};
  const char* names[3] = {"snap_dec_lds<0>", "snap_dec_lds<1>", "snap_dec_wave(sim)"};
  uint32_t hdr[2];
  int rec = 0, bad = 0, refused = 0;
  while (fread(hdr, 4, 2, f) == 2) {
    uint32_t n = hdr[0], rawlen = hdr[1];
    bool malformed = rawlen == 0xffffffffu;
    std::vector<uint8_t> in(n + 16, 0xee), raw(malformed ? 0 : rawlen);
    if (fread(in.data(), 1, n, f) != n) return 2;
    if (!malformed && rawlen && fread(raw.data(), 1, rawlen, f) != rawlen) return 2;
    // capacity as on the device: the size announced by the stream's preamble
    uint32_t cap = 0;
    for (uint32_t i = 0, s = 0; i < 5 && i < n; i++, s += 7) {
      cap |= (uint32_t)(in[i] & 0x7f) << s;
      if (!(in[i] & 0x80)) break;
    }
    if (cap > (64u << 20)) cap = 64u << 20;
    for (int d = 0; d < 3; d++) {
      std::vector<uint8_t> out((size_t)cap + 16, 0xdd);
      uint32_t r = decs[d](in.data(), n, out.data(), cap);
      if (malformed) {
        if (r != 0) { printf("rec %d: %s ACCEPTED a malformed stream\n", rec, names[d]); bad++; }
      } else if (r != rawlen || memcmp(out.data(), raw.data(), rawlen)) {
        printf("rec %d: %s MISMATCH (n=%u ulen=%u r=%u)\n", rec, names[d], n, rawlen, r);
        bad++;
      }
    }
    refused += malformed;
    rec++;
  }
  fclose(f);
  printf("corpus check: %d streams (%d malformed), %d failures\n", rec, refused, bad);
  if (bad == 0) printf("corpus check OK\n");
  return bad ? 1 : 0;
}
