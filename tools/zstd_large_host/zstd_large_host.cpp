// Runs a file of stored zstd blocks through the large-frame wave decoder of
// toplingdb_amd/csrc/dcw_zstd_dec_large.h — the very source
// k_decompress_zstd_large compiles — on the CPU, in the kernel's schedule:
// every phase between two wave barriers is a loop over lanes 0..63, the
// prefix sums are serial.  Each frame is decoded twice, with the lanes of
// every phase in ascending and in descending order: a phase that read what
// another lane of the same phase wrote would give different bytes.  Build as
// a stand-alone program with
//   g++ -O1 -g -fsanitize=address,undefined -I toplingdb_amd/csrc
//       tools/zstd_large_host/zstd_large_host.cpp -o zstd_large_host
//
//   zstd_large_host <file>
// file: records of  u32 n | u32 usize | u32 explen | n payload bytes |
// explen expected bytes.  The payload is a stored block: varint32 preamble +
// one zstd frame.  explen == 0xffffffff marks a payload that must be refused
// (by the eligibility walk or by the decoder; no expected bytes follow).
// Bit 31 of usize marks a payload that may be refused, but if decoded must
// give the bytes.
//
// The buffers are heap objects of exactly the sizes the kernel may touch, so
// the sanitizer sees any access past them: the frame plus the 7 bytes behind
// it that the staged blob guarantees, the decoded size, one work-group's
// literal scratch, one ZstdLargeLds.  Prints one line per failure,
// "refused <record>" for each payload that the walk accepted and the decoder
// refused, and a summary.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define DCW_ZSTD_WAVE
#define DCW_ZSTD_STATS
#include "dcw_zstd_dec_large.h"

using namespace dcw;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  uint32_t hdr[3];
  int rec = 0, bad = 0, malformed_n = 0, decoded = 0, nseq3 = 0;
  ZstdLargeLds* S = (ZstdLargeLds*)calloc(1, sizeof(ZstdLargeLds)); // tables persist
  uint8_t* lit = (uint8_t*)malloc(kZLitStride);
  while (fread(hdr, 4, 3, f) == 3) {
    uint32_t n = hdr[0], usize = hdr[1], explen = hdr[2];
    bool malformed = explen == 0xffffffffu;
    bool may_refuse = usize >> 31; // a changed frame that libzstd still takes
    usize &= 0x7fffffffu;
    bool has_want = !malformed && explen;
    uint8_t* payload = (uint8_t*)malloc(n ? n : 1);
    uint8_t* want = (uint8_t*)malloc(has_want ? explen : 1);
    if (fread(payload, 1, n, f) != n) return 2;
    if (has_want && fread(want, 1, explen, f) != explen) return 2;
    if (!zstd_eligible_large(payload, n)) {
      if (!malformed && !may_refuse) { printf("rec %d: walk refuses\n", rec); bad++; }
    } else {
      uint32_t us = 0;
      int hn = zstd_preamble(payload, n, &us);
      uint32_t rn = n - (uint32_t)hn;
      if (!malformed && us != usize) { printf("rec %d: usize %u\n", rec, us); bad++; }
      uint8_t* in = (uint8_t*)malloc(rn + 7);
      uint8_t* out = (uint8_t*)malloc(us ? us : 1);
      uint8_t* first = (uint8_t*)malloc(us ? us : 1);
      bool refused = false;
      for (int order = 0; order < 2; order++) {
        zw_descending = order;
        memset(in + rn, order ? 0xff : 0x00, 7);
        memcpy(in, payload + hn, rn);
        memset(out, 0xdd, us);
        memset(lit, 0xaa, kZLitStride);
        memset(zstat, 0, sizeof(zstat));
        const ZMemGlobal m = {in, out, lit};
        bool ok = zstd_dec_wave_large(*S, m, rn, us, 0);
        if ((ok ? malformed : !malformed && !may_refuse) ||
            (ok && (us != explen || memcmp(out, want, us)))) {
          printf("rec %d: order %d %s\n", rec, order, ok ? "WRONG/ACCEPTED" : "REFUSED");
          bad++;
        }
        if (ok && order == 0) memcpy(first, out, us);
        if (ok && order == 1 && memcmp(first, out, us)) {
          printf("rec %d: lane order changes the bytes\n", rec);
          bad++;
        }
        if (ok && order == 0 && zstat[ZS_NSEQ_3B]) nseq3++;
        refused |= !ok;
      }
      if (refused) printf("refused %d\n", rec);
      decoded += !refused;
      free(in);
      free(out);
      free(first);
    }
    free(payload);
    free(want);
    malformed_n += malformed;
    rec++;
  }
  fclose(f);
  free(S);
  free(lit);
  printf("zstd_large_host: %d records (%d decoded, %d malformed, %d with a 3-byte "
         "sequence count), %d failures\n", rec, decoded, malformed_n, nseq3, bad);
  if (bad == 0) printf("OK\n");
  return bad ? 1 : 0;
}
