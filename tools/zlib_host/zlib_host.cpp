// Runs a file of raw deflate streams through both decoders of
// toplingdb_amd/csrc/dcw_inflate_dec.h on the CPU: the serial inflate_dec and
// the wave decoder — the very source k_decompress_zlib compiles — in the
// kernel's schedule: every phase between two wave barriers is a loop over
// lanes 0..63.  The wave decoder runs each stream twice, with the lanes of
// every phase in ascending and in descending order: a phase that read what
// another lane of the same phase wrote would give different bytes.  Build as
// a stand-alone program with
//   g++ -O1 -g -fsanitize=address,undefined -I toplingdb_amd/csrc
//       tools/zlib_host/zlib_host.cpp -o zlib_host
//
//   zlib_host <file>
// file: records of  u32 n | u32 usize | u32 explen | n stream bytes | explen
// expected bytes.  explen == 0xffffffff marks a stream that must be refused
// (no expected bytes follow); otherwise explen == usize.
//
// The buffers are heap objects of exactly n and usize bytes, so the sanitizer
// sees any access past them.  Prints one line per failure and a summary.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define DCW_INFLATE_WAVE
#include "dcw_inflate_dec.h"

using namespace dcw;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  uint32_t hdr[3];
  int rec = 0, bad = 0, decoded = 0, refused = 0;
  uint32_t total[IS_COUNT] = {0};
  InflLds* S = (InflLds*)calloc(1, sizeof(InflLds)); // tfixed persists, as on the GPU
  while (fread(hdr, 4, 3, f) == 3) {
    const uint32_t n = hdr[0], usize = hdr[1], explen = hdr[2];
    const bool malformed = explen == 0xffffffffu;
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);
    uint8_t* want = (uint8_t*)malloc(!malformed && explen ? explen : 1);
    uint8_t* out = (uint8_t*)malloc(usize ? usize : 1);
    if (fread(in, 1, n, f) != n) return 2;
    if (!malformed && fread(want, 1, explen, f) != explen) return 2;
    bool any_ok = false;
    for (int pass = 0; pass < 3; pass++) { // serial, wave ascending, wave descending
      memset(out, 0xdd, usize);
      bool ok;
      if (pass == 0) {
        ok = inflate_dec(in, n, out, usize);
      } else {
        iw_descending = pass == 2;
        if (pass == 2) memset(istat, 0, sizeof(istat)); // count each stream once
        const InflMemGlobal m = {in, out};
        ok = infl_dec_wave(*S, m, n, usize, 0);
      }
      if (ok == malformed || (ok && (usize != explen || memcmp(out, want, usize)))) {
        printf("rec %d: pass %d %s\n", rec, pass, ok ? "WRONG/ACCEPTED" : "REFUSED");
        bad++;
      }
      any_ok |= ok;
    }
    for (int i = 0; i < IS_COUNT; i++) {
      if (i == IS_MAXLEN || i == IS_ROUNDS)
        total[i] = total[i] < istat[i] ? istat[i] : total[i];
      else
        total[i] += istat[i];
    }
    memset(istat, 0, sizeof(istat));
    decoded += any_ok;
    refused += !any_ok;
    free(in);
    free(want);
    free(out);
    rec++;
  }
  fclose(f);
  free(S);
  printf("zlib_host: %d records (%d decoded, %d refused), blocks: %u stored, %u "
         "fixed (%u table builds), %u dynamic; longest code %u; most match "
         "rounds %u; %d failures\n",
         rec, decoded, refused, total[IS_STORED], total[IS_FIXED],
         total[IS_FIXED_BUILDS], total[IS_DYNAMIC], total[IS_MAXLEN],
         total[IS_ROUNDS], bad);
  if (bad == 0) printf("OK\n");
  return bad ? 1 : 0;
}
