// Runs a file of stored zstd blocks through the wave decoder of
// toplingdb_amd/csrc/dcw_zstd_dec.h — the very source k_decompress_zstd
// compiles — on the CPU, in the kernel's schedule: every phase between two
// wave barriers is a loop over lanes 0..63, the prefix sums are serial.
// Each frame is decoded twice, with the lanes of every phase in ascending and
// in descending order: a phase that read what another lane of the same phase
// wrote would give different bytes.  Build as a stand-alone program with
//   g++ -O1 -g -fsanitize=address,undefined -I toplingdb_amd/csrc
//       tools/zstd_host/zstd_host.cpp -o zstd_host
//
//   zstd_host <file>
// file: records of  u32 n | u32 usize | u32 explen | n payload bytes |
// explen expected bytes.  The payload is a stored block: varint32 preamble +
// one zstd frame.  explen == 0xffffffff marks a payload that must be refused
// (by the eligibility walk or by the decoder), 0xfffffffe one that the walk
// must leave to the host (no expected bytes follow either).  Bit 31 of usize
// marks a payload that may be refused, but if decoded must give the bytes.
//
// The ZstdWave and the payload copy are heap objects of exactly the kernel's
// sizes, so the sanitizer sees any access past them.  Prints one line per
// failure, "refused-eligible <record>" for each must-refuse payload that
// passed the walk and was refused by the decoder, and how many records
// exercised each format mode.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define DCW_ZSTD_WAVE
#define DCW_ZSTD_STATS
#include "dcw_zstd_dec.h"

using namespace dcw;

static const char* kStatNames[ZS_COUNT] = {
    "block_raw", "block_rle", "block_compressed",
    "lit_raw", "lit_rle", "lit_huf1", "lit_huf4", "lit_treeless",
    "weights_direct", "weights_fse",
    "ll_predefined", "ll_rle", "ll_fse", "ll_repeat",
    "of_predefined", "of_rle", "of_fse", "of_repeat",
    "ml_predefined", "ml_rle", "ml_fse", "ml_repeat",
    "rep1_ll0", "rep2_ll0", "rep3_ll0", "rep1", "rep2", "rep3",
    "nseq_0", "nseq_1byte", "nseq_2byte", "nseq_3byte", "overlap_match"};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  uint32_t hdr[3], modes[ZS_COUNT] = {0};
  int rec = 0, bad = 0, refused = 0, host_only = 0, decoded = 0;
  ZstdWave* S = (ZstdWave*)calloc(1, sizeof(ZstdWave)); // tables persist
  while (fread(hdr, 4, 3, f) == 3) {
    uint32_t n = hdr[0], usize = hdr[1], explen = hdr[2];
    bool malformed = explen == 0xffffffffu, to_host = explen == 0xfffffffeu;
    bool may_refuse = usize >> 31; // a changed frame that libzstd still takes
    usize &= 0x7fffffffu;
    bool has_want = !malformed && !to_host && explen;
    uint8_t* payload = (uint8_t*)malloc(n ? n : 1);
    uint8_t* want = (uint8_t*)malloc(has_want ? explen : 1);
    if (fread(payload, 1, n, f) != n) return 2;
    if (has_want && fread(want, 1, explen, f) != explen) return 2;
    bool elig = zstd_eligible(payload, n);
    if (!elig) {
      if (!malformed && !to_host) { printf("rec %d: walk says host-only\n", rec); bad++; }
      host_only += to_host;
    } else if (to_host) {
      printf("rec %d: walk accepted a host-only block\n", rec);
      bad++;
    } else {
      uint32_t us = 0;
      int hn = zstd_preamble(payload, n, &us);
      uint32_t rn = n - (uint32_t)hn;
      if (!malformed && us != usize) { printf("rec %d: usize %u\n", rec, us); bad++; }
      uint8_t first[kZstdMax];
      for (int order = 0; order < 2; order++) {
        zw_descending = order;
        memset(S->in, order ? 0xff : 0x00, sizeof(S->in));
        memset(S->out, 0xdd, sizeof(S->out));
        memcpy(S->in, payload + hn, rn);
        memset(zstat, 0, sizeof(zstat));
        bool ok = zstd_dec_wave(*S, rn, us, 0);
        if ((ok ? malformed : !malformed && !may_refuse) ||
            (ok && (us != explen || memcmp(S->out, want, us)))) {
          printf("rec %d: order %d %s\n", rec, order, ok ? "WRONG/ACCEPTED" : "REFUSED");
          bad++;
        }
        if (ok && order == 0) memcpy(first, S->out, us);
        if (ok && order == 1 && memcmp(first, S->out, us)) {
          printf("rec %d: lane order changes the bytes\n", rec);
          bad++;
        }
        if (order == 0)
          for (int m = 0; m < ZS_COUNT; m++) modes[m] += zstat[m] != 0;
      }
      if (malformed) printf("refused-eligible %d\n", rec);
      decoded += !malformed;
    }
    free(payload);
    free(want);
    refused += malformed;
    rec++;
  }
  fclose(f);
  free(S);
  for (int m = 0; m < ZS_COUNT; m++) printf("mode %s %u\n", kStatNames[m], modes[m]);
  printf("zstd_host: %d records (%d decoded, %d malformed, %d host-only), %d failures\n",
         rec, decoded, refused, host_only, bad);
  if (bad == 0) printf("OK\n");
  return bad ? 1 : 0;
}
