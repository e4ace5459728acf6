// Runs a file of preset dictionaries and stored zstd blocks through
// toplingdb_amd/csrc/dcw_zstd_dict.h — the very source k_zstd_dict_prepare,
// k_decompress_zstd_dict and k_decompress_zstd_large_dict compile — on the
// CPU, in the kernels' schedule: every phase between two wave barriers is a
// loop over lanes 0..63.  Dictionary preparation and every frame run twice,
// with the lanes of every phase ascending and descending; the two runs must
// agree byte for byte.  Build as a stand-alone program with
//   g++ -O1 -g -fsanitize=address,undefined -I toplingdb_amd/csrc
//       tools/zstd_dict_host/zstd_dict_host.cpp -o zstd_dict_host
//
//   zstd_dict_host <file>
// file: records of  u32 n | u32 usize | u32 explen | n payload bytes | explen
// expected bytes, as tools/zstd_host reads them (explen == 0xffffffff: must be
// refused).  A record with usize == 0xfffffffe is a dictionary (n bytes, no
// expected bytes; n == 0: none) for the records behind it.  A block goes to
// the small decoder if zstd_eligible() takes it, else to the large one if
// zstd_eligible_large() does, as in the worker.
//
// Dictionary, record, frame (+ the 7 bytes behind it that the staged blob
// guarantees to the large decoder), output and states are heap objects of
// exactly the sizes the kernels may touch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define DCW_ZSTD_WAVE
#include "dcw_zstd_dict.h"

using namespace dcw;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  uint32_t hdr[3];
  int rec = 0, bad = 0, malformed_n = 0, decoded = 0, small_n = 0, large_n = 0;
  int dicts = 0, dicts_refused = 0;
  ZstdWave* SW = (ZstdWave*)calloc(1, sizeof(ZstdWave));
  ZstdLargeLds* SL = (ZstdLargeLds*)calloc(1, sizeof(ZstdLargeLds));
  ZstdDictTables* T = (ZstdDictTables*)calloc(2, sizeof(ZstdDictTables));
  uint8_t* lit = (uint8_t*)malloc(kZLitStride);
  uint8_t* dict = nullptr;
  uint32_t dict_n = 0;
  while (fread(hdr, 4, 3, f) == 3) {
    uint32_t n = hdr[0], usize = hdr[1], explen = hdr[2];
    if (usize == 0xfffffffeu) { // a dictionary
      free(dict);
      dict = n ? (uint8_t*)malloc(n) : nullptr;
      dict_n = n;
      if (n && fread(dict, 1, n, f) != n) return 2;
      for (int order = 0; order < 2 && n; order++) {
        zw_descending = order;
        memset(&T[order], order ? 0xff : 0x00, sizeof(ZstdDictTables));
        T[order].fail = 0;
        zstd_dict_prepare(*SL, dict, n, &T[order], 0);
      }
      if (n && T[0].fail != T[1].fail) { printf("dict %d: lane order\n", dicts); bad++; }
      if (n && !T[0].fail) {
        // a raw dictionary leaves the tables alone; a full one fills all of
        // the record in front of its last four words (full .. fail)
        size_t cmp = T[0].full ? sizeof(ZstdDictTables) - 16 : 0;
        if (memcmp(&T[0], &T[1], cmp) || T[0].content_off != T[1].content_off ||
            T[0].content_len != T[1].content_len || T[0].full != T[1].full) {
          printf("dict %d: lane order changes the tables\n", dicts);
          bad++;
        }
      }
      dicts_refused += n && T[0].fail;
      dicts++;
      continue;
    }
    bool malformed = explen == 0xffffffffu;
    bool has_want = !malformed && explen;
    uint8_t* payload = (uint8_t*)malloc(n ? n : 1);
    uint8_t* want = (uint8_t*)malloc(has_want ? explen : 1);
    if (fread(payload, 1, n, f) != n) return 2;
    if (has_want && fread(want, 1, explen, f) != explen) return 2;
    const bool small = zstd_eligible(payload, n, dict_n != 0);
    const bool large = !small && zstd_eligible_large(payload, n, dict_n != 0);
    if (!small && !large) {
      if (!malformed) { printf("rec %d: walks refuse\n", rec); bad++; }
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
        const ZstdDictTables* Tp = dict_n ? &T[order] : nullptr;
        bool ok;
        uint8_t* got = out;
        if (small) {
          memset(SW->in, order ? 0xff : 0x00, sizeof(SW->in));
          memset(SW->out, 0xdd, sizeof(SW->out));
          memcpy(SW->in, payload + hn, rn);
          ok = zstd_dec_wave_dict(*SW, Tp, dict, rn, us, 0);
          got = SW->out;
        } else {
          memset(in + rn, order ? 0xff : 0x00, 7);
          memcpy(in, payload + hn, rn);
          memset(out, 0xdd, us);
          memset(lit, 0xaa, kZLitStride);
          const ZMemGlobal m = {in, out, lit};
          ok = zstd_dec_wave_large_dict(*SL, m, Tp, dict, rn, us, 0);
        }
        if (ok == malformed || (ok && (us != explen || memcmp(got, want, us)))) {
          printf("rec %d: order %d %s\n", rec, order, ok ? "WRONG/ACCEPTED" : "REFUSED");
          bad++;
        }
        if (ok && order == 0) memcpy(first, got, us);
        if (ok && order == 1 && memcmp(first, got, us)) {
          printf("rec %d: lane order changes the bytes\n", rec);
          bad++;
        }
        refused |= !ok;
      }
      decoded += !refused;
      small_n += small;
      large_n += large;
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
  free(SW); free(SL); free(T); free(lit); free(dict);
  printf("zstd_dict_host: %d dictionaries (%d refused), %d records (%d decoded, "
         "%d malformed, %d small, %d large), %d failures\n",
         dicts, dicts_refused, rec, decoded, malformed_n, small_n, large_n, bad);
  if (bad == 0) printf("OK\n");
  return bad ? 1 : 0;
}
